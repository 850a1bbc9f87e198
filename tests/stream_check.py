"""The stream contract of include/neddf_hip.h, checked on a side stream (helper of tests/test_gpu_streams.py, not a test module).

Every stage call promises to run asynchronously on the stream it is given; a named handful synchronise that stream to read a count.
On the default stream every mistake against that promise -- a launch, memset or copy on the null stream, a count read that did not
wait, a device-wide synchronise in a warm call -- still gives the right answer.  `StreamCheck.run` makes the mistake visible:

  reference   the call on the default stream with its inputs resident, twice: the first call sizes every workspace (a growing
              workspace synchronises the device, capi_internal.h `ensure`), the second is timed -- host wall time of the call alone
              and of call plus synchronise -- and must reproduce the first bit for bit
  stale       the call once more on the default stream with ALL-ZERO inputs, result dropped: the context's workspaces now hold the
              intermediates of the zero inputs, so a stray launch that reads a workspace early finds no leftover of the right answer
  late        fresh input buffers full of zero bytes and a device synchronise; then on the side stream, with no host synchronisation
              in between: event a, a spinning kernel, event b, blocks of the outputs' sizes filled with a sentinel byte and handed
              back to the side stream's allocator pool, where the wrapper's own output buffers then come from (best effort: the
              wrappers allocate their outputs themselves), the real inputs copied in from device-resident staging copies, the call,
              a clone of every output, event c; the side stream is synchronised last.  The sentinel lands behind the delay: what a
              stray launch or memset wrote into an output early is overwritten by it
  verdict     the clones are the reference outputs bit for bit (host-returned counts: equal).  An entry point the header does not
              document as synchronising has returned to the host while b was still pending: it was enqueued while its inputs did not
              exist yet and it did not block the host.  One that is documented as synchronising returns after b: it waited for its
              count

The delay is one spinning kernel (torch.cuda._sleep), calibrated once per StreamCheck from an event pair, its length set against
the reference run: at least 50 times the host time of the call alone, for a synchronising call at least 10 times the time of call
plus synchronise (a stray kernel starts within microseconds of its enqueue: any delay that outlasts the enqueue is enough, the factor
covers host jitter), never below 20 ms -- a guess at host jitter, not a measurement -- and never above 200 ms: a case whose rule
asks for more needs a smaller shape.  A realised delay (a to b) below the rule, or b fired before an asynchronous call returned, is
"inconclusive: delay too short" and fails.  Nothing here retries, skips or sleeps.

Only leaf data is delivered late -- coordinates, rays, volumes, densities, gradients, flags, the vertices and indices of a build.
Structures that kernels walk (trees, cell lists, index lists) are built in an earlier step and compared with the default-stream
build (`same_structure`) before anything traverses them.  No buffer is ever filled with NaN patterns or wild indices.
"""
import time

import torch

FLOOR_MS, CAP_MS = 20.0, 200.0       # the floor is a guess at host jitter on a loaded host, stated as such
FACTOR_CALL, FACTOR_SYNC = 50.0, 10.0
SENTINEL = 0x5A                      # byte pattern: float32 1.5e16, int32 1515870810 -- nothing a case computes


class Inconclusive(AssertionError):
    pass


def delay_rule(call_ms, sync_ms, synchronising):
    """The delay in ms that the reference timings ask for (docstring above); AssertionError above the cap."""
    want = max(FLOOR_MS, FACTOR_CALL * call_ms, FACTOR_SYNC * sync_ms if synchronising else 0.0)
    assert want <= CAP_MS, "the delay rule asks for %.1f ms (call %.3f ms, call + synchronise %.3f ms): above %g ms, the case needs a smaller shape" % (
        want, call_ms, sync_ms, CAP_MS)
    return want


def flatten(out, prefix="out"):
    """[(name, tensor or host value)] of a nested tuple / list / dict result, in a fixed order."""
    if isinstance(out, torch.Tensor) or out is None or isinstance(out, (int, float, bool, str)):
        return [(prefix, out)]
    if hasattr(out, "item") and getattr(out, "ndim", 1) == 0:      # a numpy scalar
        return [(prefix, out.item())]
    if isinstance(out, dict):
        return [p for k in sorted(out) for p in flatten(out[k], "%s.%s" % (prefix, k))]
    if isinstance(out, (tuple, list)):
        return [p for i, v in enumerate(out) for p in flatten(v, "%s[%d]" % (prefix, i))]
    raise TypeError("stream_check: a result of type %s" % type(out).__name__)


def same_bits(a, b):
    """Two tensors of one dtype and shape with the same bytes (the int32-view comparison of tests/test_gpu_raycast.py, for any dtype)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)))


def compare(got, ref, what):
    """None, or the first difference between two flattened results as a message."""
    if [n for n, _ in got] != [n for n, _ in ref]:
        return "%s: result layout %s != %s" % (what, [n for n, _ in got], [n for n, _ in ref])
    for (name, a), (_, b) in zip(got, ref):
        if isinstance(b, torch.Tensor):
            if not isinstance(a, torch.Tensor) or not same_bits(a, b):
                if isinstance(a, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype:
                    bad = int((a.contiguous().view(-1).view(torch.uint8) != b.contiguous().view(-1).view(torch.uint8)).sum().item())
                    return "%s: %s differs from the default-stream result in %d of %d bytes" % (what, name, bad, b.numel() * b.element_size())
                return "%s: %s is %s, the default-stream result %s %s" % (
                    what, name, "%s %s" % (a.dtype, tuple(a.shape)) if isinstance(a, torch.Tensor) else repr(a), b.dtype, tuple(b.shape))
        elif a != b and not (isinstance(a, float) and isinstance(b, float) and a != a and b != b):
            return "%s: host value %s is %r, on the default stream %r" % (what, name, a, b)
    return None


def within_reordering(got, ref, n_terms, what):
    """Outputs that floating-point atomics sum in an order that changes from run to run -- the parameter gradients of the training
    kernels, one term per sample point, added across workgroups -- have no bits to compare.  The bound comes from the number
    format: an fp32 sum of N terms evaluated in two orders differs by at most 2 (N - 1) 2^-24 sum |x_i| (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2).  sum |x_i| of an element cannot be seen from outside; it is taken to be at most
    G, the largest |gradient| of its tensor on the default stream -- true of every element whose terms do not cancel, and the elements
    whose terms cancel are the small ones.  Per tensor: |got - ref| <= N 2^-23 G, N = n_terms (2.7e-5 G for 229 points).  Not a measured
    number.  A mis-ordered launch sums other terms (zero upstream gradients give zeros) and is off by the order of G itself.
    None, or the first violation as a message."""
    for (name, a), (_, b) in zip(got, ref):
        if a is None or b is None:
            if a is not b:
                return "%s: %s is %s, on the default stream %s" % (what, name, type(a).__name__, type(b).__name__)
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: %s is %s %s, on the default stream %s %s" % (what, name, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
        if a.numel() == 0:
            continue
        x, y = a.double(), b.double()
        tol = n_terms * 2.0 ** -23 * float(y.abs().max())
        bad = ~((x - y).abs() <= tol)           # a NaN is outside
        if bool(bad.any()):
            return "%s: %s differs from the default-stream result by up to %.3e in %d of %d elements (bound %.3e = %d * 2^-23 * %.3e)" % (
                what, name, float((x - y).abs()[bad].nan_to_num(float("inf")).max()), int(bad.sum()), a.numel(), tol, n_terms, float(y.abs().max()))
    return None


def sort_lists(start, items):
    """The items of every list in ascending order: `start` int32 [L + 1] offsets, items int32 [start[L]] -- the canonical form of a
    grid whose lists are filled by integer atomics (include/neddf_hip.h: the order INSIDE a list may depend on timing)."""
    counts = (start[1:] - start[:-1]).long()
    lists = torch.repeat_interleave(torch.arange(counts.shape[0], device=start.device), counts)
    assert lists.shape[0] == items.shape[0], "the offsets do not describe the item list"
    key = (lists << 32) | items.long()
    return (torch.sort(key).values & 0xFFFFFFFF).to(torch.int32)


def same_structure(built, ref, what):
    """Asserts that a structure built on a side stream (already synchronised) is the default-stream build bit for bit; nothing
    traverses it before."""
    msg = compare(flatten(built), flatten(ref), what)
    assert msg is None, msg


class StreamCheck:
    """One side stream (a second for the cases that need two), a calibrated spinning kernel and the records of every run."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.side = torch.cuda.Stream(self.device)
        self.side2 = torch.cuda.Stream(self.device)
        self.records = []
        self.controls = None          # None: not run; "" : passed; a message otherwise
        self.dead = None              # the error that ended a run other than by an assertion: no case starts anything after it
        self._cycles_per_ms = self._calibrate()

    def _calibrate(self):
        torch.cuda.synchronize(self.device)
        torch.cuda._sleep(1000)                   # first launch of the kernel
        best = None
        for cycles in (2_000_000, 20_000_000):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            best = cycles / max(a.elapsed_time(b), 1e-3)
        return best

    def enqueue_delay(self, ms):
        """The spinning kernel for `ms` milliseconds (and a quarter: the calibration is an estimate) on the current stream."""
        torch.cuda._sleep(int(self._cycles_per_ms * ms * 1.25))

    def require_controls(self):
        if self.dead is not None:
            raise Inconclusive("inconclusive: an earlier case ended in an error (%s); nothing more is started on the device" % self.dead)
        if self.controls is None:
            raise Inconclusive("inconclusive: the controls have not run")
        if self.controls:
            raise Inconclusive("inconclusive: a control failed, the harness could not have detected anything (%s)" % self.controls)

    # ------------------------------------------------------------------ the three steps
    def run(self, name, fn, late, **kw):
        """_run, and after an error that is no assertion -- a HIP error, say -- every later case reports inconclusive instead of
        starting more work on a device that may have faulted."""
        try:
            return self._run(name, fn, late, **kw)
        except AssertionError:
            raise
        except Exception as e:
            if type(e).__name__ == "NeddfError" and "(code -2)" not in str(e):      # the library refused the call: no device error
                raise
            self.dead = "%s: %s: %s" % (name, type(e).__name__, str(e)[:200])
            raise

    def _run(self, name, fn, late, synchronising=False, stream=None, check_async=True, stale=True, canon=None, reordered=None, n_terms=0):
        """fn(*tensors) -> result (nested tuples / dicts of tensors and host values) with `late`, a list of device tensors, delivered
        late.  fn must not keep or change `late` itself: it is handed copies (an entry point that changes an input in place returns
        that input among its results).  synchronising: the header documents a stream synchronise.  check_async=False: no assertion
        on when the call returns (Python-layer functions, which legitimately read counts).  canon: result -> result, applied before
        every comparison, for outputs that the header documents as depending on timing (the order inside a cell's list).  reordered:
        a predicate on the flattened names of the outputs that are NOT repeatable run to run on any stream -- sums of n_terms terms by
        floating-point atomics -- which are held to the bound of a reordered sum instead (`within_reordering`).  Returns the record."""
        self.require_controls()
        side = self.side if stream is None else stream
        dev = self.device
        canon = canon or (lambda out: out)
        loose = reordered or (lambda n: False)

        def snapshot(out):
            got = [(n, v.clone() if isinstance(v, torch.Tensor) else v) for n, v in flatten(canon(out))]
            return [p for p in got if not loose(p[0])], [p for p in got if loose(p[0])]
        # (a) reference: warm-up, then the timed run
        warm, warm_loose = snapshot(fn(*[t.clone() for t in late]))
        torch.cuda.synchronize(dev)
        inputs = [t.clone() for t in late]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn(*inputs)
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        ref, ref_loose = snapshot(out)
        del out
        call_ms, sync_ms = (t1 - t0) * 1e3, (t2 - t0) * 1e3
        msg = compare(ref, warm, name + " (two default-stream runs)") or within_reordering(ref_loose, warm_loose, n_terms, name + " (two default-stream runs)")
        assert msg is None, msg
        want_ms = delay_rule(call_ms, sync_ms, synchronising)
        # stale workspaces: what a stray early launch would find
        if stale and late:
            try:
                fn(*[torch.zeros_like(t) for t in late])
            except RuntimeError:
                pass                    # an error return on all-zero inputs is an answer too; the late run must still match
            torch.cuda.synchronize(dev)
        # (b) late inputs
        staging = [t.clone() for t in late]
        zeroed = [torch.zeros_like(t) for t in late]
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            a.record()
            self.enqueue_delay(want_ms)
            b.record()
            # behind the delay, so that what a stray launch or memset wrote early is overwritten too
            parked = [torch.empty(v.numel() * v.element_size(), device=dev, dtype=torch.uint8).fill_(SENTINEL)
                      for _, v in ref + ref_loose if isinstance(v, torch.Tensor) and v.numel()]
            del parked                  # back into this stream's pool: the call's own torch.empty of these sizes lands on them
            for z, s in zip(zeroed, staging):
                z.copy_(s)
            h0 = time.perf_counter()
            out = fn(*zeroed)
            h1 = time.perf_counter()
            fired = b.query()
            got, got_loose = snapshot(out)
            c.record()
        side.synchronize()
        realised = a.elapsed_time(b)
        rec = dict(name=name, call_ms=call_ms, call_sync_ms=sync_ms, delay_ms=want_ms, realised_ms=realised, late_call_ms=(h1 - h0) * 1e3,
                   synchronising=synchronising, returned_before_b=not fired, total_ms=a.elapsed_time(c))
        self.records.append(rec)
        print("stream_check %-40s call %.3f ms  call+sync %.3f ms  delay chosen %.1f ms  realised %.1f ms  late call %.3f ms  %s" % (
            name, call_ms, sync_ms, want_ms, realised, rec["late_call_ms"], "synchronising" if synchronising else "asynchronous"))
        # (c) verdict
        if realised < want_ms:
            raise Inconclusive("inconclusive: delay too short (%s: realised %.2f ms, the rule asks for %.2f ms)" % (name, realised, want_ms))
        msg = compare(got, ref, name + " on a side stream with late inputs") or within_reordering(got_loose, ref_loose, n_terms, name + " on a side stream with late inputs")
        assert msg is None, msg
        if check_async and not synchronising:
            if fired and rec["late_call_ms"] < 0.5 * want_ms:
                raise Inconclusive("inconclusive: delay too short (%s: the delay had ended when the call returned after %.3f ms)" % (name, rec["late_call_ms"]))
            assert not fired, ("%s is not documented as synchronising, but it returned after %.2f ms, when the %.1f ms delay ahead of it on its stream "
                               "had ended: it blocked the host" % (name, rec["late_call_ms"], want_ms))
        if check_async and synchronising:
            assert fired, "%s is documented as synchronising its stream, but it returned while the work ahead of it was pending" % name
        return rec

    def build_on_side(self, name, build, ref, canon=None):
        """A structure built under the side stream from resident inputs, synchronised and compared with `ref`, the default-stream
        build (both through `canon`, see run); returns it."""
        self.require_controls()
        canon = canon or (lambda out: out)
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(self.side):
            built = build()
        self.side.synchronize()
        same_structure(canon(built), canon(ref), name + " built on a side stream")
        return built


class Recorder:
    """ctx.lib with every neddf_* function that is called noted in `calls`."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("neddf_"):
            return fn
        calls = self._calls

        def recorded(*args):
            calls.add(name)
            return fn(*args)
        return recorded
