"""The launch plan of the field kernels (neddf_amd/csrc/field_plan.h) on the CPU: how field_forward cuts N points into chunks (one
colour launch and one hand-off each) and a chunk into distance launches, and how the free-memory probe shrinks a chunk.  A launch
that crossed its chunk would write past a hand-off buffer sized for `chunk` points.  A stand-alone driver (tests/capi/field_plan.cpp)
runs the plan and the walk field_forward makes under AddressSanitizer + UBSan over the sweep below; the result is held to the
invariants and to a restatement of the rules in Python integers."""
import itertools
import os
import subprocess

import pytest
from conftest import ROOT

NS = (1, 63, 2**16, 2**16 + 1, 2**19, 2**19 + 1, 2**20, 2**20 + 81, 2**23, 2**23 + 1, 3 * 2**23 + 5, 2**25 + 1)
ENVS = (0, 12, 16, 20, 30)                 # 0: NEDDF_FIELD_CHUNK_LOG2 not set; 12 clamps to 16, 30 to 25
AUX_ROW = 64                               # 16 floats of per-point record
FLOOR = 2**16


def rows(full):
    """(features, record) bytes per hand-off point at engine width 256: one row of fp32 features eval-minimal, four with the Jacobian"""
    return (4 if full else 1) * 256 * 4, AUX_ROW


def need(chunk, per_point):
    return chunk * per_point + chunk * per_point // 8


FREE = ("ample", "below_2^23", "floor", "failed")


def free_bytes(kind, per_point):
    if kind == "below_2^23":               # a quarter of it is one byte short of a 2^23-point hand-off
        return 4 * need(2**23, per_point) - 1
    return {"ample": 2**46, "floor": 0, "failed": 2**46}[kind]


CACHES = ("empty", "same_row", "other_row")
CAPS = ("zero", "fits", "fits_2^18")        # fits: no probe; fits_2^18: a probe above 2^18 points, and own blocks to count as free


def cases():
    for N, full, use3, env, free, cache, caps in itertools.product(NS, (0, 1), (0, 1), ENVS, FREE, CACHES, CAPS):
        feat_row, aux_row = rows(full)
        pp = feat_row + aux_row
        cap_points = {"zero": 0, "fits": 2**25, "fits_2^18": 2**18}[caps]
        cache_row, cache_chunk = {"empty": (0, 0), "same_row": (pp, 2**18), "other_row": (pp + 64, 2**18)}[cache]
        yield dict(N=N, full=full, use3=use3, env=env, free=free, cache=cache, caps=caps, feat_row=feat_row, aux_row=aux_row,
                   feat_cap=cap_points * feat_row, aux_cap=cap_points * aux_row, cache_row=cache_row, cache_chunk=cache_chunk,
                   probe_ok=int(free != "failed"), free_b=free_bytes(free, pp))


def rule(c):
    """The rules of the plan, restated: (chunk, ddf_sub, probed, cache)"""
    env = 0 if not c["env"] else min(max(c["env"], 16), 25)
    ddf_sub = 2**20 if c["use3"] and not env else 2**25
    cap = 2**19 if c["full"] else 2**(env or 23)
    chunk = min(c["N"], cap)
    pp = c["feat_row"] + c["aux_row"]
    if c["cache_row"] == pp and c["cache_chunk"] > 0:
        chunk = min(chunk, c["cache_chunk"])               # an earlier settled chunk for the same row size stands
    probed = c["feat_cap"] < chunk * c["feat_row"] or c["aux_cap"] < chunk * c["aux_row"]     # only when a buffer would have to grow
    asked = chunk
    if probed and c["probe_ok"]:
        free = c["free_b"] + c["feat_cap"] + c["aux_cap"]
        while chunk > FLOOR and need(chunk, pp) > free // 4:
            chunk //= 2
    return chunk, ddf_sub, int(probed), int(chunk < asked)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """[(case, chunk, ddf_sub, probed, cache, probes, walk)], walk = [(off, n, [(so, n_sub)])]: one compile, one run of the driver"""
    tmp = tmp_path_factory.mktemp("fieldplan")
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    exe, case_file = str(tmp / "field_plan"), str(tmp / "cases.txt")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g",
                           "-I", csrc, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "capi", "field_plan.cpp"), "-o", exe])
    all_cases = list(cases())
    with open(case_file, "w") as f:
        for c in all_cases:
            f.write("%(full)d %(use3)d %(N)d %(env)d %(feat_row)d %(aux_row)d %(feat_cap)d %(aux_cap)d %(cache_row)d %(cache_chunk)d "
                    "%(probe_ok)d %(free_b)d\n" % c)
    p = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not any(s in p.stderr for s in ("Sanitizer", "runtime error")), p.stderr[-4000:]
    lines = p.stdout.strip().split("\n")
    assert len(lines) == len(all_cases)
    out = []
    for c, line in zip(all_cases, lines):
        v = line.split()
        head, walk, subs = [int(x) for x in v[:5]], [], []
        assert (len(v) - 5) % 3 == 0, line[:200]
        for kind, a, b in zip(v[5::3], v[6::3], v[7::3]):
            if kind == "D":
                subs.append((int(a), int(b)))
            else:
                assert kind == "C", line[:200]
                walk.append((int(a), int(b), subs))
                subs = []
        assert not subs, "distance launches behind the last colour launch: " + line[:200]
        out.append((c, *head, walk))
    return out


def outcome(c, chunk, probed, cache):
    if not probed:
        return "no probe"
    if not c["probe_ok"]:
        return "probe failed"
    if not cache:
        return "probe kept the chunk"
    return "floor" if chunk == FLOOR else "probe shrank the chunk"


def test_sweep_covers_every_policy_triple_and_every_free_memory_outcome(plans):
    assert {(c["full"], c["use3"], c["env"]) for c, *_ in plans} == set(itertools.product((0, 1), (0, 1), ENVS))
    assert {(c["N"], c["free"], c["cache"], c["caps"]) for c, *_ in plans} == set(itertools.product(NS, FREE, CACHES, CAPS))
    assert {outcome(c, chunk, probed, cache) for c, chunk, _, probed, cache, _, _ in plans} == \
        {"no probe", "probe failed", "probe kept the chunk", "probe shrank the chunk", "floor"}
    # the free-memory classes do what their names say where nothing else decides: eval-minimal, no override, nothing cached or held
    for c, chunk, _, probed, cache, _, _ in plans:
        if c["N"] >= 2**23 and not c["full"] and not c["env"] and c["cache"] == "empty" and c["caps"] == "zero":
            assert (chunk, probed, cache) == {"ample": (2**23, 1, 0), "below_2^23": (2**22, 1, 1), "floor": (FLOOR, 1, 1),
                                              "failed": (2**23, 1, 0)}[c["free"]], c
    assert any(len(walk) > 1 for *_, walk in plans) and any(len(subs) > 1 for *_, walk in plans for _, _, subs in walk)


def test_plan_equals_the_restated_rules(plans):
    for c, chunk, ddf_sub, probed, cache, probes, _ in plans:
        assert (chunk, ddf_sub, probed, cache) == rule(c), c
        assert probes == probed, c                          # the probe runs once when the plan says so, and never otherwise


def test_launches_tile_the_points_and_stay_inside_their_chunk(plans):
    for c, chunk, ddf_sub, _, _, _, walk in plans:
        at = 0
        for off, n, subs in walk:                           # one entry per colour launch: exactly one per chunk
            assert off == at and 1 <= n <= chunk, (c, off, n)
            at += n
            sat = 0
            for so, n_sub in subs:
                assert so == sat and 1 <= n_sub <= ddf_sub, (c, off, so, n_sub)
                sat += n_sub
                assert so + n_sub <= n, (c, off, so, n_sub)  # every hand-off offset stays inside the buffer sized for `chunk`
            assert sat == n, (c, off)
        assert at == c["N"], c
        assert len(walk) == -(-c["N"] // chunk), c


def test_cache_and_probe_conditions(plans):
    for c, chunk, _, probed, cache, _, _ in plans:
        asked = rule(dict(c, probe_ok=0))[0]                # what the plan asks for before the probe
        assert cache == int(probed and c["probe_ok"] and chunk < asked), c     # written only when the probe shrank the chunk
        if c["feat_cap"] >= asked * c["feat_row"] and c["aux_cap"] >= asked * c["aux_row"]:
            assert not probed and chunk == asked, c         # no probe when the buffers already fit
        assert chunk == asked or 2 * chunk >= FLOOR, c    # only a chunk above the floor is halved (2^16 + 1 points become 2^15)
