"""numpy restatement of the packed weight layout (neddf_amd/csrc/kernels.h LayerW, field_pack.hip) for tests/test_pack_host.py:
case files for tests/capi/pack_dump.cpp, the parser of what it writes, the unpacking of a fragment-major block back to a dense [K][N]
matrix, and the matrices / vectors / scalars every argument block has to hold, built from the state tensors by the reference's own
concatenation order (neddf.py: cat([embed_pos, h]); nerf.py / neus.py: cat([h, embed_pos]))."""
import struct

import numpy as np

NEDDF, NERF, NEUS = 0, 1, 2
MAX_LAYERS, MAX_STASH = 12, 4


def roundup(x, m):
    return (x + m - 1) // m * m


def desc(kind, E, Ed, layers, width, col_layers=0, col_width=0, skips=(), activation=2, density_activation=0, d_near=0.01, dtype=0):
    return dict(kind=kind, E=E, Ed=Ed, layers=layers, width=width, col_layers=col_layers, col_width=col_width, skips=tuple(skips),
                activation=activation, density_activation=density_activation, d_near=d_near,
                penalty_weight=(0.5, 0.25, 1.0, 2.0, 0.125, 4.0), penalty_has=(1, 0, 1, 1, 0, 1), dtype=dtype)


def tensor_shapes(d):
    """[(weight shape, bias count)] in the order neddf_set_field documents (include/neddf_hip.h)."""
    Cpe, Cdir, W, skips = 6 * d["E"], 6 * d["Ed"], d["width"], d["skips"]
    cin = lambda l: Cpe if l == 0 else W + (Cpe if (l - 1) in skips else 0)
    if d["kind"] == NEDDF:       # LinearGradLayer: [in, out]
        nt, nc = d["layers"] - 1, d["col_layers"] - 1
        return [((cin(l), W), W) for l in range(nt)] + [((Cpe + Cdir + 3 + W if l == 0 else W, W), W) for l in range(nc)] + \
               [((W, 1), 1), ((W, 1), 1), ((W, 3), 3)]
    if d["kind"] == NERF:        # nn.Linear: [out, in]
        return [((W, cin(l)), W) for l in range(d["layers"])] + [((1, W), 1), ((W // 2, W + Cdir), W // 2), ((3, W // 2), 3)]
    Wc = d["col_width"]
    return [((W, cin(l)), W) for l in range(d["layers"])] + [((Wc, 6 + Cdir + W if l == 0 else Wc), Wc) for l in range(d["col_layers"])] + \
           [((3, Wc), 3), ((1, 1), 1)]


def random_tensors(d, seed):
    rng = np.random.default_rng(seed)
    shapes = tensor_shapes(d)
    return ([rng.uniform(-0.9, 0.9, s).astype(np.float32) for s, _ in shapes], [rng.uniform(-0.9, 0.9, n).astype(np.float32) for _, n in shapes])


def write_case(path, d, W, B, n_tensors=None):
    skips = list(d["skips"]) + [0] * (8 - len(d["skips"]))
    head = struct.pack("<8i8i2if6f6ii", d["kind"], d["E"], d["Ed"], d["layers"], d["width"], d["col_layers"], d["col_width"], len(d["skips"]),
                       *skips, d["activation"], d["density_activation"], d["d_near"], *d["penalty_weight"], *d["penalty_has"], d["dtype"])
    assert len(head) == 128
    with open(path, "wb") as f:
        f.write(head + struct.pack("<2i", len(W) if n_tensors is None else n_tensors, len(W)))
        for w, b in zip(W, B):
            f.write(struct.pack("<2i", w.size, b.size) + np.ascontiguousarray(w, np.float32).tobytes() + np.ascontiguousarray(b, np.float32).tobytes())


def parse_out(path):
    raw = open(path, "rb").read()
    text, blob = raw.split(b"end\n", 1)
    out = dict(M={}, V={}, N=set(), S={}, blob=np.frombuffer(blob, np.float32))
    for line in text.decode().splitlines():
        tag, _, rest = line.partition(" ")
        if tag in ("rc", "has3", "blob"):
            out[tag + ("_len" if tag == "blob" else "")] = int(rest)
        elif tag == "err":
            out["err"] = rest
        elif tag == "N":
            out["N"].add(rest)
        elif tag == "S":
            name, v = rest.split()
            out["S"][name] = np.array([int(v[1:], 16)], np.uint32).view(np.float32)[0] if v[0] == "f" else int(v)
        else:
            name, *v = rest.split()
            out[tag][name] = tuple(int(x) for x in v)        # M: offset, super-steps, columns, operand policy; V: offset, floats
    return out


# ---- the layout, from the formula in kernels.h: wp[(((tile * ksteps + S) * 64 + lane) * planes + plane) * half + r] =
#      W[k = step * S + half * (lane >> 5) + r][n = tile * 32 + (lane & 31)], step = 8 (fp32) or 16 (16-bit policies), half = step / 2
PLANES = {0: 1, 1: 1, 2: 2, 3: 3}


def block_floats(ksteps, cols, operands):
    step = 16 if operands else 8
    return ksteps * step * cols * (PLANES[operands] if operands else 2) // 2


def unpack(blob, off, ksteps, cols, operands):
    """-> [planes][K][N] of uint32 (fp32) or uint16 (16-bit policies) bit patterns"""
    half, planes, tiles = (8 if operands else 4), PLANES[operands], cols // 32
    words = blob[off:off + block_floats(ksteps, cols, operands)].view(np.uint16 if operands else np.uint32)
    a = words.reshape(tiles, ksteps, 2, 32, planes, half)           # tile, super-step, lane half, lane & 31, plane, r
    return a.transpose(4, 1, 2, 5, 0, 3).reshape(planes, ksteps * 2 * half, cols)


def bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def check_block(planes, want, operands):
    """planes: what unpack() returned; want: the dense fp32 matrix the block stands for"""
    want = np.ascontiguousarray(want, np.float32)
    if operands == 0:
        assert np.array_equal(planes[0], want.view(np.uint32))                                  # bit for bit
    elif operands == 1:
        assert np.array_equal(planes[0], bf16_rne(want))                                        # round to nearest even
    elif operands == 3:
        total = sum(bf16_value(p).astype(np.float64) for p in planes)
        assert np.array_equal(total, want.astype(np.float64))                                   # hi + mid + lo == w exactly
    else:
        sv = want * np.float32(1024.0)
        h = sv.astype(np.float16)                                                               # to nearest ...
        over = np.abs(h.astype(np.float32)) > np.abs(sv)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)                                   # ... then back toward zero
        m = (sv - h.astype(np.float32)).astype(np.float16)                                      # nearest half of what is left
        assert np.array_equal(planes[0], h.view(np.uint16)) and np.array_equal(planes[1], m.view(np.uint16))


# ---- what the argument blocks have to hold
def enc_rows(rank, K, base):
    """engine columns of the [sin half | cos half] encoding -> feature index of the layer's input (-1: padding)"""
    return [base + q if q < 3 * rank else -1 for q in range(K)] + [base + 3 * rank + q if q < 3 * rank else -1 for q in range(K)]


def hidden_rows(width, WP, base):
    return [base + k if k < width else -1 for k in range(WP)]


def dense(Wlog, rows, cols, step):
    """[K][N]: engine column k reads input feature rows[k] of the logical [in][out] matrix; zero rows / columns of padding"""
    rows = np.array(list(rows) + [-1] * (-len(rows) % step))
    out = np.zeros((len(rows), cols), np.float32)
    out[rows >= 0, :Wlog.shape[1]] = Wlog[rows[rows >= 0]]
    return out


def pad(v, n):
    out = np.zeros(n, np.float32)
    out[:v.size] = v.reshape(-1)
    return out


def engine_width(width, d):
    w = roundup(width, 128)
    while w < 2 * roundup(3 * d["E"], 4) + 2 * roundup(3 * d["Ed"], 4) + 32:
        w += 128
    return w


class Expect:
    """M: name -> dense [K][N]; V: name -> vector; S: name -> scalar -- of one argument-block set under one operand policy"""

    def __init__(self, d, operands):
        self.d, self.operands, self.step = d, operands, 16 if operands else 8
        self.M, self.V, self.S = {}, {}, {}
        self.KH, self.KD, self.Cpe, self.Cdir = roundup(3 * d["E"], 4), roundup(3 * d["Ed"], 4), 6 * d["E"], 6 * d["Ed"]

    def mat(self, name, Wlog, rows, cols):
        self.M[name] = dense(Wlog, rows, cols, self.step)
        return self.M[name].shape[0] // self.step

    def trunk(self, a, Wlog, B, n, width, WP, enc_first):
        d, n_stash, self.stash_of = self.d, 0, {}
        for l in range(n):
            wide = l > 0 and (l - 1) in d["skips"]
            rows = enc_rows(d["E"], self.KH, 0) if l == 0 else hidden_rows(width, WP, self.Cpe if wide and enc_first else 0)
            self.S["%s.layer[%d].ksteps" % (a, l)] = self.mat("%s.layer[%d].wp" % (a, l), Wlog[l], rows, WP)
            self.S["%s.layer[%d].stash" % (a, l)] = n_stash if wide else -1
            if wide:
                self.S["%s.stash[%d].ksteps" % (a, n_stash)] = self.mat("%s.stash[%d].wp" % (a, n_stash), Wlog[l],
                                                                         enc_rows(d["E"], self.KH, 0 if enc_first else width), WP)
                self.S["%s.stash[%d].col0" % (a, n_stash)] = 0
                self.stash_of[l] = n_stash
                n_stash += 1
            self.V["%s.layer[%d].bias" % (a, l)] = pad(B[l], WP)
        self.S.update({a + ".n_layers": n, a + ".n_stash": n_stash, a + ".width": WP, a + ".operands": self.operands, a + ".activation": d["activation"]})

    def transposes(self, a, Wlog, n, width, WP, enc_first):
        """engine-column order: B[k][n] = W_l[input row0 + n][output k] (hidden part), B[k][j] = W_l[encoding column j's feature][k] (64 wide)"""
        def pe_T(name, Wl, base):
            out = np.zeros((WP, 64), np.float32)
            for j, r in enumerate(enc_rows(self.d["E"], self.KH, base)):
                if r >= 0:
                    out[:width, j] = Wl[r]
            self.M[name] = out
        skip_layer = -1
        for l in range(1, n):
            wide = (l - 1) in self.d["skips"]
            row0 = self.Cpe if wide and enc_first else 0
            out = np.zeros((WP, WP), np.float32)
            out[:width, :width] = Wlog[l][row0:row0 + width].T
            self.M["%s.wT[%d]" % (a, l)] = out
            if wide:
                skip_layer = l
                pe_T("%s.wT_pe_skip[%d]" % (a, self.stash_of[l]), Wlog[l], 0 if enc_first else width)
        pe_T(a + ".wT_pe0", Wlog[0], 0)
        self.S.update({a + ".skip_layer": skip_layer, a + ".ks_hidden": WP // self.step})

    def col_trunk(self, c, Wlog, B, n, small, feat_row, feat, width, WP):
        self.S[c + ".ksteps_a"] = self.mat(c + ".wp_a", Wlog[0], small, WP)
        for l in range(n):
            rows = hidden_rows(feat, WP, feat_row) if l == 0 else hidden_rows(width, WP, 0)
            self.S["%s.layer[%d].ksteps" % (c, l)] = self.mat("%s.layer[%d].wp" % (c, l), Wlog[l], rows, WP)
            self.S["%s.layer[%d].stash" % (c, l)] = -1
            self.V["%s.layer[%d].bias" % (c, l)] = pad(B[l], WP)
        self.S.update({c + ".n_layers": n, c + ".width": WP, c + ".operands": self.operands, c + ".activation": self.d["activation"]})


def expect_neddf(d, W, B, operands, a="ddf", c="col"):
    e = Expect(d, operands)
    nt, nc, Wd = d["layers"] - 1, d["col_layers"] - 1, d["width"]
    WP = engine_width(Wd, d)
    e.trunk(a, W, B, nt, Wd, WP, True)
    e.V[a + ".w_ddf_out"], e.V[a + ".w_aux_out"] = pad(W[nt + nc], WP), pad(W[nt + nc + 1], WP)
    e.transposes(a, W, nt, Wd, WP, True)
    small = enc_rows(d["E"], e.KH, 0) + enc_rows(d["Ed"], e.KD, e.Cpe) + [e.Cpe + e.Cdir + k for k in range(3)]
    e.col_trunk(c, W[nt:], B[nt:], nc, small, e.Cpe + e.Cdir + 3, Wd, Wd, WP)
    e.V[c + ".w_out"] = pad(W[nt + nc + 2], 3 * WP)                                   # [Wd][3] -> [WP][3]
    e.S.update({a + ".b_ddf_out": B[nt + nc][0], a + ".b_aux_out": B[nt + nc + 1][0], a + ".d_near": np.float32(d["d_near"]), a + ".neus": 0,
                a + ".density_activation": d["density_activation"], c + ".mode": 0, c + ".final_act": -1})
    for k in range(3):
        e.S["%s.b_out[%d]" % (c, k)] = B[nt + nc + 2][k]
    for k in range(6):
        e.S["%s.penalty_weight[%d]" % (c, k)], e.S["%s.penalty_has[%d]" % (c, k)] = np.float32(d["penalty_weight"][k]), d["penalty_has"][k]
    return e


def expect_neus(d, W, B, operands):
    e = Expect(d, operands)
    ns, nc, Ws, Wc = d["layers"], d["col_layers"], d["width"], d["col_width"]
    WP = engine_width(max(Ws, Wc), d)
    Wlog = [w.T for w in W[:ns + nc + 1]]
    e.trunk("ddf", Wlog, B, ns, Ws, WP, False)
    e.transposes("ddf", Wlog, ns, Ws, WP, False)
    e0 = np.zeros(WP, np.float32)
    e0[0] = 1.0
    e.V["ddf.w_ddf_out"], e.V["ddf.w_aux_out"] = e0, np.zeros(WP, np.float32)        # the sdf is feature 0 of the last layer; no aux head
    small = [0, 1, 2] + [3 + e.Cdir + k for k in range(3)] + [-1, -1] + enc_rows(d["Ed"], e.KD, 3)      # [pos | gradient | pad 2 | dir]
    e.col_trunk("col", Wlog[ns:], B[ns:], nc, small, 6 + e.Cdir, Ws, Wc, WP)
    e.V["col.w_out"] = pad(np.ascontiguousarray(Wlog[ns + nc]), 3 * WP)              # [3][Wc] -> [WP][3]
    e.S.update({"ddf.b_ddf_out": np.float32(0), "ddf.b_aux_out": np.float32(0), "ddf.neus": 1, "ddf.neus_v10": W[ns + nc + 1].reshape(-1)[0] * np.float32(10.0),
                "col.mode": 1, "col.final_act": d["activation"]})
    for k in range(3):
        e.S["col.b_out[%d]" % k] = B[ns + nc][k]
    return e


def expect_nerf(d, W, B, operands):
    e = Expect(d, operands)
    n, Wn = d["layers"], d["width"]
    WP, Wh = engine_width(Wn, d), Wn // 2
    HC = roundup(max(Wh, 1), 128)
    Wlog = [w.T for w in W]
    e.trunk("nerf", Wlog, B, n, Wn, WP, False)
    s = e.S["nerf.n_stash"]                                                             # the colour head's direction segment: one more stash slot
    e.V["nerf.w_density"] = pad(W[n], WP)
    e.S["nerf.col0.ksteps"] = e.mat("nerf.col0.wp", Wlog[n + 1], hidden_rows(Wn, WP, 0), HC)
    e.S["nerf.stash[%d].ksteps" % s] = e.mat("nerf.stash[%d].wp" % s, Wlog[n + 1], enc_rows(d["Ed"], e.KD, Wn), HC)
    e.V["nerf.col0.bias"] = pad(B[n + 1], HC)
    w1 = np.zeros((3, HC), np.float32)
    w1[:, :Wh] = W[n + 2]
    e.V["nerf.w_col1"] = w1.reshape(-1)
    e.S.update({"nerf.n_stash": s + 1, "nerf.col_stash": s, "nerf.col0.stash": s, "nerf.stash[%d].col0" % s: roundup(2 * e.KH, e.step),
                "nerf.b_density": B[n][0], "nerf.density_activation": d["density_activation"]})
    for k in range(3):
        e.S["nerf.b_col1[%d]" % k] = B[n + 2][k]
    return e


def expected(d, W, B, split3):
    """the Expect of every argument-block set pack_field fills for this descriptor"""
    if d["kind"] == NEDDF:
        sets = [expect_neddf(d, W, B, d["dtype"])]
        if d["dtype"] == 0 and split3:
            sets.append(expect_neddf(d, W, B, 3, "ddf3", "col3"))
        return sets
    return [(expect_nerf if d["kind"] == NERF else expect_neus)(d, W, B, d["dtype"])]


def check(out, d, W, B, split3=True):
    """everything tests/test_pack_host.py asks of one accepted case"""
    assert out["rc"] == 0 and out["err"] == "", (out["rc"], out["err"])
    sets = expected(d, W, B, split3)
    assert out["has3"] == (len(sets) == 2)
    blob, spans = out["blob"], []
    assert out["blob_len"] == blob.size
    want_ptrs = set()
    for e in sets:
        for name, want in e.M.items():
            assert name in out["M"], "%s is null or missing" % name
            off, ks, cols, operands = out["M"][name]
            assert (ks * e.step, cols, operands) == (want.shape[0], want.shape[1], e.operands), (name, out["M"][name], want.shape)
            assert off % 64 == 0 and 0 <= off and off + block_floats(ks, cols, operands) <= blob.size, name
            spans.append((off, off + block_floats(ks, cols, operands), name))
            try:
                check_block(unpack(blob, off, ks, cols, operands), want, operands)
            except AssertionError:
                raise AssertionError("%s differs from the state tensors under operand policy %d" % (name, operands))
        for name, want in e.V.items():
            assert name in out["V"], "%s is null or missing" % name
            off, n = out["V"][name]
            assert n == want.size and off % 64 == 0 and 0 <= off and off + n <= blob.size, (name, off, n, want.size)
            spans.append((off, off + n, name))
            assert np.array_equal(blob[off:off + n].view(np.uint32), want.view(np.uint32)), name
        for name, want in e.S.items():
            got = out["S"][name]
            same = np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32) if isinstance(want, np.floating) else got == want
            assert same, (name, got, want)
        want_ptrs |= set(e.M) | set(e.V)
    # a pointer is bound exactly when the kernels of this kind read it; blocks do not overlap
    assert set(out["M"]) | set(out["V"]) == want_ptrs, (set(out["M"]) | set(out["V"])) ^ want_ptrs
    spans.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, "%s and %s overlap" % (an, bn)
    for name, v in out["S"].items():
        if name.endswith(".caller_pointers"):
            assert v == 0, name
