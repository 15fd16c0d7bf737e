"""Range probes: sampling networks in the oracle's layout whose every matrix sum has ONE non-zero term (probe_networks.sampling_probe's form),
extended from "weights +-1, bias 0" to chosen gains and chosen constants, so that what a 16-bit sampling engine returns is its operand
rounding at the edges of the operand range and nothing else: fp16 subnormals, hi = 0 with lo' carrying, ties in either conversion, weights
whose hi part is subnormal or zero, the last finite values below 65520.  numpy only.

A probe carries up to min(128, width // 2) entries, one output column each (outputs past them are 0).  Entry kinds:
  ("const", c)              one unit: layer-0 weights 0 and bias c -- the hidden activation is relu(c) on every ray;
  ("const", c, m)           the same, carried through hidden layer 1 with weight m (a "gain on a known value");
  ("ray", col, g)           two units u+ = relu(+g f), u- = relu(-g f), f = input column col (an identity column of the encoding);
                            the output is u+ - u-, and one of the two is 0 on every ray;
  ("ray", col, g, m)        the same with weight m in hidden layer 1.
Middle layers carry each unit on with weight 1 (their place moves from layer to layer, probe_networks._places: first and last unit of the
width included, so output tile 0 and the tile handed on as PendingTile3 both carry units); the last layer is +1 (u-: -1).  Every other
weight and bias is 0.

predict(): what an engine returns, from the inputs alone, written per layer as the kernels write it (k_sampling16.hip.hpp):
  split   acc = bias + Whi xhi; cross = Whi xlo' + Wlo' xhi; v = fma(cross, 2^-11, acc) in fp32; ReLU that keeps a NaN; (hi, lo') =
          split_parts(v); the last layer returns v.  Weights are split as the packer splits them (pack.cpp F16_SPLIT: the same rule).
  fp16    acc = bias + fp16(W) fp16(x); ReLU; one conversion to fp16.
  fp32    fp32(bias + W x), the bits.
The fp16 conversion is numpy's: round to nearest even, subnormals kept, inf from 65520 on.  Where Wlo' is 0, or xlo' is 0, `cross` has one
non-zero term as well and the prediction is one bit pattern.  Where both are non-zero, `cross` takes ONE rounding inside the matrix pipe
whose form is not documented: predict(..., rnd="down" / "up") round that sum toward -inf / +inf (an exact sum rounded to fp32, never a
tolerance), everything behind it is monotone (a chain has at most one such layer, and only weights +-1 behind it: range_probe asserts it),
so the output lies between the two predictions (bracket()).  rnd="rne" is the round-to-nearest value, for the records.  In fact the
bracket never opens on fp32 inputs: x and W hold 24 bits, so lo' has its last bit at 2^-12 of hi's first or above, each cross product its
last bit at 2^-22 of |W x| or above and the sum at most 24 bits -- exact in fp32 whatever the pipe does.  The comparison keeps the bracket
form so that nothing rests on this argument; the records show how many entries it decided (none so far: every entry by equality).
A ray is BAD where an operand of some layer is not finite (an activation >= 65520, a NaN or infinite bias; fp32: a non-finite value): the
engine's row is then non-finite in EVERY column (0 x inf = NaN in every other unit, ReLU keeps it), and that is all the prediction says.

fault=...: emulated wrong kernels (tests/test_sampling_ranges_cpu.py shows each rejected by named entries)."""
import numpy as np

import mlp_reference as M
import probe_networks as P

W, H = P.W, P.H
F16_EDGE = np.float32(65520.0)                 # the smallest value fp16 rounds to inf
LAST_BELOW_EDGE = np.nextafter(F16_EDGE, np.float32(0))
TINY16 = 2.0 ** -14                            # the smallest normal fp16
FAULTS = ("ftz", "rtz_hi", "rtz_lo", "double_lo", "saturate", "no_cross", "no_wlo", "relu_nan0")


def _p(e):
    return float(np.ldexp(1.0, e))


# ---- the constants table ------------------------------------------------------------------------------------------------------------------

AROUND_ONE = [("1", 1.0), ("1+2^-10", 1 + _p(-10)), ("1+2^-11", 1 + _p(-11)), ("1+3*2^-11", 1 + 3 * _p(-11)),
              ("1+2^-11+2^-23", 1 + _p(-11) + _p(-23)), ("1+2^-22", 1 + _p(-22)), ("1+2^-23", 1 + _p(-23)),
              ("1+2^-11-2^-23", 1 + _p(-11) - _p(-23))]
SUBNORMAL_HI = [("2^-14", _p(-14)), ("2^-14-2^-24", _p(-14) - _p(-24)), ("2^-24", _p(-24)), ("3*2^-25", 3 * _p(-25)), ("1e-5", 1e-5)]
ZERO_HI = [("2^-25", _p(-25)), ("2^-25+2^-40", _p(-25) + _p(-40)), ("2^-26", _p(-26)), ("1e-8", 1e-8), ("2^-35", _p(-35)), ("2^-36", _p(-36)),
           ("2^-36+2^-50", _p(-36) + _p(-50)), ("2^-37", _p(-37)), ("2^-126", _p(-126))]
TOP = [("32768", 32768.0), ("65504", 65504.0), ("65512", 65512.0), ("nextafter(65520,0)", float(LAST_BELOW_EDGE))]
# the split engine holds nextafter(65520, 0) as hi = 65504, lo' = fp16(32760) = 32768 (a tie, to even): the value 65520 itself, which the next
# layer's conversion turns into inf.  65520 - 2^-7 is the last fp32 whose lo' stays 32752
TOP_SPLIT = TOP[:3] + [("65520-2^-7", 65520.0 - _p(-7))]
OVERFLOW = [("65520", 65520.0), ("1e5", 1e5), ("3e38", 3e38), ("+inf", float("inf")), ("nan", float("nan"))]
OVERFLOW_FINITE32 = OVERFLOW[:3]               # the same without the two values no matrix product carries (0 x inf = NaN in every engine)

GAINS = [("2^-13", _p(-13)), ("2^-20", _p(-20)), ("2^-30", _p(-30)), ("2^-37", _p(-37)), ("1/3", float(np.float32(1.0 / 3.0))),
         ("pi", float(np.float32(np.pi))), ("2^15", 32768.0), ("65000", 65000.0)]
GAIN_OVER = [("65520", 65520.0), ("1e5", 1e5)]      # a sampling weight outside the fp16 range: pack.cpp packs hi = inf, lo' = -inf


def table_entries():
    """the finite part of the table below the top of the range: the positive values, -0.0 and every value negated (ReLU gives +0), and the
    gains on a known value: 0.75 (fp16 holds it: xlo' = 0, so Wlo' xhi is the only cross term and the prediction is exact) and 1 + 2^-22
    (both cross terms: the bracket)"""
    pos = AROUND_ONE + SUBNORMAL_HI + ZERO_HI
    ent = [(n, ("const", v)) for n, v in pos] + [("-0.0", ("const", -0.0))] + [("-(" + n + ")", ("const", -v)) for n, v in pos + TOP]
    ent += [("0.75 x " + n, ("const", 0.75, g)) for n, g in GAINS] + [("(1+2^-22) x " + n, ("const", 1 + _p(-22), g)) for n, g in GAINS[4:6]]
    return ent


def const_entries(table):
    return [(n, ("const", v)) for n, v in table]


def ray_entries(dir_cols, pos_cols, feat):
    """every gain on every identity column it keeps inside the fp16 range on the rows `feat` (g max|f| < 65504; asserted again on the
    device's own rows by whoever predicts: a BAD ray there is a test failure)"""
    ent = []
    for c in list(dir_cols) + list(pos_cols):
        top = float(np.abs(np.asarray(feat)[:, c]).max())
        for n, g in GAINS:
            if g * top < 65504.0:
                ent.append(("%s x f[%d]" % (n, c), ("ray", int(c), g)))
    return ent


def edge_probes(dir_cols, feat):
    """[entries]: one probe per direction column whose ray-driven activation crosses 65520 inside the frame -- 2^15 f through a second gain m
    (both fp16-exact: one bit pattern), m = 1, 1.25, 1.5 or 1.75 times the power of two that puts the share of rays beyond the edge nearest to
    one half -- beside the constants around 1, which have to come out exact on every ray that stays inside.  One such entry per probe: a ray
    is lost to any of them."""
    out = []
    for c in dir_cols:
        a = np.abs(np.asarray(feat, np.float64)[:, c]) * 32768.0
        best = None
        for k in range(-2, 14):
            for f in (1.0, 1.25, 1.5, 1.75):
                m = f * _p(k)
                share = float((a * m >= float(F16_EDGE)).mean())
                if best is None or abs(share - 0.5) < abs(best[0] - 0.5):
                    best = (share, m)
        out.append([("2^15 f[%d] x %g" % (c, best[1]), ("ray", int(c), 32768.0, best[1]))] + const_entries(AROUND_ONE))
    return out


def chunks(entries, width):
    per = min(128, width // 2)
    return [entries[i:i + per] for i in range(0, len(entries), per)]


# ---- the probe ----------------------------------------------------------------------------------------------------------------------------

def _split32(x):
    with np.errstate(over="ignore", invalid="ignore"):      # a weight outside the fp16 range: (inf, -inf)
        hi, lo = M.split_parts(np.float32(x))
    return float(hi), float(lo)


def range_probe(n_in, depth, width, entries, seed=0, bins=128):
    """entries: [(name, spec)] -> (net0 in the oracle's layout (fp32), chains).  chains[j]: for output j the list of its units, each a dict
    (col or None, w [depth] fp32 weights along the chain, b: layer-0 bias, place [depth - 1]: its unit index per hidden layer)."""
    k = len(entries)
    assert depth >= 3 and 1 <= k <= min(128, width // 2) and k <= bins
    specs = [s for _, s in entries]
    n_units = sum(1 if s[0] == "const" else 2 for s in specs)
    rng = np.random.default_rng(seed)
    place = P._places(rng, depth - 1, width, n_units) if n_units > 1 else [np.array([(7 * i) % width]) for i in range(depth - 1)]
    dims = [n_in] + [width] * (depth - 1) + [bins]
    net = {}
    for i in range(depth):
        net["layers.%d.weight" % i] = np.zeros((dims[i + 1], dims[i]), np.float32)
        net["layers.%d.bias" % i] = np.zeros(dims[i + 1], np.float32)
    chains, u = [], 0
    for j, s in enumerate(specs):
        units = []
        if s[0] == "const":
            mid = np.float32(s[2]) if len(s) > 2 else np.float32(1.0)
            units.append(dict(col=None, w0=np.float32(0.0), b=np.float32(s[1]), mid=mid, last=np.float32(1.0)))
        else:
            assert s[0] == "ray" and 0 <= s[1] < n_in, s
            mid = np.float32(s[3]) if len(s) > 3 else np.float32(1.0)
            for sg in (1.0, -1.0):
                units.append(dict(col=int(s[1]), w0=np.float32(sg * s[2]), b=np.float32(0.0), mid=mid, last=np.float32(sg)))
        for un in units:
            un["place"] = [int(place[i][u]) for i in range(depth - 1)]
            un["w"] = [un["w0"], un["mid"]] + [np.float32(1.0)] * (depth - 3) + [un["last"]]
            # one non-zero term per sum: a weighted unit has no bias; at most one layer of the chain has a weight with Wlo' != 0, and only
            # weights +-1 stand behind it (the bracket's monotonicity)
            assert un["b"] == 0 or un["w0"] == 0
            inexact = [i for i, w in enumerate(un["w"]) if _split32(w)[1] != 0.0]
            assert len(inexact) <= 1 and (not inexact or all(abs(w) == 1.0 for w in un["w"][inexact[0] + 1:])), (s, un["w"])
            if un["col"] is not None:
                net["layers.0.weight"][un["place"][0], un["col"]] = un["w0"]
            net["layers.0.bias"][un["place"][0]] = un["b"]
            net["layers.1.weight"][un["place"][1], un["place"][0]] = un["mid"]
            for i in range(2, depth - 1):
                net["layers.%d.weight" % i][un["place"][i], un["place"][i - 1]] = 1.0
            net["layers.%d.weight" % (depth - 1)][j, un["place"][depth - 2]] = un["last"]
            u += 1
        chains.append(units)
    assert u == n_units
    return net, chains


def tiles_visited(chains, width):
    """per hidden layer the set of 32-unit output tiles that carry a unit (a 256-wide layer: tile 7 is the pending tile)"""
    depth1 = len(chains[0][0]["place"])
    return [sorted({un["place"][i] // 32 for ch in chains for un in ch}) for i in range(depth1)]


# ---- the rounding model, per layer --------------------------------------------------------------------------------------------------------

def _f16(x, fault=None, which="hi"):
    """fp32 array -> fp16 values as float64 under the model (RNE, subnormals kept, inf from 65520) or an emulated fault of this conversion"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if fault == "rtz_" + which:
            h = M._rtz(x, "fp16")
            h = np.where(np.isfinite(x), h, x.astype(np.float64))
        elif fault == "double_lo" and which == "lo":
            # first to 11 significant bits with the exponent unbounded, then to fp16's grid: differs on a subnormal result only
            m, e = np.frexp(x.astype(np.float64))
            h = np.where(np.isfinite(x), np.ldexp(np.rint(m * 2048.0), e - 11), x).astype(np.float32).astype(np.float16).astype(np.float64)
        else:
            h = x.astype(np.float16).astype(np.float64)
        if fault == "saturate":
            h = np.where(np.isinf(h) & np.isfinite(x), np.sign(x) * 65504.0, h)
        if fault == "ftz":
            h = np.where(np.abs(h) < TINY16, np.copysign(0.0, h), h)
    return h


def _parts(x, fault=None):
    """(hi, lo') of split_pack / the packer's F16_SPLIT arm, as float64"""
    x = np.asarray(x, np.float32)
    hi = _f16(x, fault, "hi")
    with np.errstate(over="ignore", invalid="ignore"):
        r = ((x - hi.astype(np.float32)) * np.float32(M.SPLIT)).astype(np.float32)      # exact in fp32
    return hi, _f16(r, fault, "lo")


def _sum_f32(a, b, rnd="rne"):
    """fp32 of the exact sum of two float64 arrays, rounded ONCE: to nearest even, or toward -inf ("down") / +inf ("up").  The sum is first
    rounded to odd in float64 (TwoSum tells whether it was exact), which keeps every later rounding that of the exact sum."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        s = a + b
        bb = s - a
        err = (a - (s - bb)) + (b - bb)
        ok = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        s = np.where(ok & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        f = s.astype(np.float32)
        if rnd == "down":
            f = np.where(np.isfinite(s) & (f.astype(np.float64) > s), np.nextafter(f, np.float32(-np.inf)), f)
        elif rnd == "up":
            f = np.where(np.isfinite(s) & (f.astype(np.float64) < s), np.nextafter(f, np.float32(np.inf)), f)
        else:
            assert rnd == "rne", rnd
    return f.astype(np.float32)


def _relu(v, fault=None):
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        out = np.where(v > 0, v, np.float32(0.0))
    return out if fault == "relu_nan0" else np.where(nan, v, out).astype(np.float32)


def _layer(x, w, b, engine, rnd, fault):
    """one unit of one layer: x [n] fp32 (the previous activation, before it is made an operand), w, b fp32 scalars -> (v [n] fp32, finite [n]:
    every operand was finite)"""
    x = np.asarray(x, np.float32)
    w, b = np.float32(w), np.float32(b)
    with np.errstate(over="ignore", invalid="ignore"):
        if engine == "fp32":
            v = _sum_f32(x.astype(np.float64) * np.float64(w), np.float64(b))
            return v, np.isfinite(x) & np.isfinite(w)
        if engine == "fp16":
            xq, wq = _f16(x, fault), _f16(w, fault)
            return _sum_f32(xq * wq, np.float64(b)), np.isfinite(xq) & np.isfinite(wq)
        assert engine == "split", engine
        xh, xl = _parts(x, fault)
        wh, wl = _parts(w, fault)
        if fault == "no_wlo":
            wl = np.float64(0.0)
        acc = _sum_f32(wh * xh, np.float64(b))                      # one of the two is 0: exact
        cross = _sum_f32(wh * xl, wl * xh, rnd)                     # the one sum that can round inside the matrix pipe
        if fault == "no_cross":
            cross = np.zeros_like(cross)
        v = _sum_f32(cross.astype(np.float64) * (1.0 / M.SPLIT), acc.astype(np.float64))
        return v, np.isfinite(xh) & np.isfinite(xl) & np.isfinite(wh) & np.isfinite(wl)


def predict(feat, chains, engine, rnd="rne", fault=None, hidden=None):
    """feat [n, n_in] fp32 -> (out [n, k] fp32, bad [n] bool).  bad: an operand or an output of some unit is not finite -- under a fault: an
    output is not finite (what the faulty kernel would show).  hidden: a list that receives, per chain unit, the layer-0 activation (fp32)"""
    feat = np.asarray(feat, np.float32)
    n = feat.shape[0]
    out = np.zeros((n, len(chains)), np.float32)
    bad_op, bad_out = np.zeros(n, bool), np.zeros(n, bool)
    for j, units in enumerate(chains):
        parts = []
        for un in units:
            x = feat[:, un["col"]] if un["col"] is not None else np.zeros(n, np.float32)
            depth = len(un["w"])
            for i in range(depth):
                v, fin = _layer(x, un["w"][i], un["b"] if i == 0 else 0.0, engine, rnd, fault)
                bad_op |= ~fin
                if i + 1 < depth:
                    x = _relu(v, fault)
                    if i == 0 and hidden is not None:
                        hidden.append(x)
                else:
                    bad_out |= ~np.isfinite(v)
                    parts.append(v)
        if len(parts) == 1:
            out[:, j] = parts[0]
        else:      # u+ - u-: one of the two is +-0 on every ray; the accumulator starts at the bias +0, so a zero sum is +0
            with np.errstate(invalid="ignore"):
                out[:, j] = _sum_f32(parts[0].astype(np.float64), parts[1].astype(np.float64))
    return out, (bad_out if fault is not None else bad_op | bad_out)


def bracket(feat, chains, engine):
    """-> (lo, hi, rne [n, k] fp32, bad [n]): the output lies in [lo, hi]; lo == hi (bit for bit) wherever no sum rounds inside the pipe"""
    d, bad = predict(feat, chains, engine, "down")
    u, bad_u = predict(feat, chains, engine, "up")
    r, bad_r = predict(feat, chains, engine, "rne")
    assert np.array_equal(bad, bad_u) and np.array_equal(bad, bad_r)
    with np.errstate(invalid="ignore"):
        lo, hi = np.minimum(d, u), np.maximum(d, u)
        assert ((r >= lo) & (r <= hi))[~bad].all()
    return lo, hi, r, bad


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(rows, lo, hi, rne, bad):
    """rows [n, k] against a bracket -> dict: wrong [n, k] (outside, or a BAD ray with a finite column, or a good ray's non-finite column),
    and the counts the records hold: exact (lo == hi) / bracketed entries, and of the bracketed ones how many sat at lo, at hi, at rne"""
    rows = np.asarray(rows, np.float32)
    good = ~bad[:, None]
    eq = bits(lo) == bits(hi)
    with np.errstate(invalid="ignore"):
        inside = np.where(eq, bits(rows) == bits(lo), (rows >= lo) & (rows <= hi))
    wrong = np.where(good, ~inside, np.isfinite(rows))
    br = good & ~eq
    return dict(wrong=wrong, checked=int(good.sum()) * 1, by_equality=int((good & eq).sum()), by_bracket=int(br.sum()),
                at_lower=int((br & (bits(rows) == bits(lo))).sum()), at_upper=int((br & (bits(rows) == bits(hi))).sum()),
                at_rne=int((br & (bits(rows) == bits(rne))).sum()), bad_rays=int(bad.sum()))


# ---- classes of the ray-driven activations --------------------------------------------------------------------------------------------------

# the least share of the frame's rays on which at least one ray-driven unit's layer-0 activation falls into the band (the split model's
# (hi, lo') of it).  Conditions on the construction, met by the oracle's features (tests/test_sampling_ranges_cpu.py) and asserted on the
# device's own rows.  lo_zero counts activations other than 0 (the idle unit of every pair is 0 on every ray and would meet any floor):
# hi holds such a value alone, so it is rare among products g f -- the gain 2^-37 (packs to 0) is not counted either.  The oracle's frame
# gives 0.061 there and 1.0 in every other band (each has a gain that puts every ray into it).
FLOORS = dict(hi_subnormal=0.90, hi_zero_lo_carries=0.90, lo_subnormal=0.90, big=0.90, lo_zero=0.03)


def class_flags(feat, chains):
    """-> {band: [n] bool, a ray-driven unit of this probe is in the band on the ray}; from the features alone"""
    hid = []
    predict(feat, chains, "split", hidden=hid)
    units = [un for ch in chains for un in ch]
    fl = {k: np.zeros(np.asarray(feat).shape[0], bool) for k in FLOORS}
    for un, x in zip(units, hid):
        if un["col"] is None:
            continue
        hi, lo = _parts(x)
        fl["hi_subnormal"] |= (hi != 0) & (np.abs(hi) < TINY16)
        fl["hi_zero_lo_carries"] |= (hi == 0) & (lo != 0)
        fl["lo_subnormal"] |= (lo != 0) & (np.abs(lo) < TINY16)
        fl["lo_zero"] |= (lo == 0) & (x != 0)
        fl["big"] |= x >= 32768.0
    return fl


def class_shares(flags):
    """flags: one class_flags() per probe of a frame -> {band: share of rays with a unit of some probe in the band}"""
    return {k: float(np.any([f[k] for f in flags], axis=0).mean()) for k in FLOORS}


def check_floors(shares, what):
    for k, floor in FLOORS.items():
        assert shares[k] >= floor, "%s: band %s holds %.4f of the rays (floor %.4f)" % (what, k, shares[k], floor)


# ---- the packed weights, as mfma_emulation reads them ---------------------------------------------------------------------------------------

def slot_columns_layer0(fp, fd):
    """[(half, slot)] -> input column of the oracle's layout, for layer 0's slots [PE(dir) | PE(pos)] (mfma_emulation.pe_eval): -1 = padding"""
    from mfma_emulation import pe_slots
    cols = {}
    base_col, base_slot = 0, 0
    for F in (fd, fp):
        for q in range(pe_slots(F)):
            for h in range(2):
                c = -1
                if q < 3 * F:
                    b, comp = divmod(q, 3)
                    c = 3 + 6 * b + (3 if h else 0) + comp
                elif q == 3 * F:
                    c = 2 if h else 0
                elif q == 3 * F + 1 and h == 0:
                    c = 1
                cols[h, base_slot + q] = base_col + c if c >= 0 else -1
        base_col += 3 + 6 * F
        base_slot += pe_slots(F)
    return cols


def dense_weights(w, lay, l, precision, n_cols, col_of):
    """the packed fragments of layer record l (mfma_emulation.PackedNet.layer / layer_split's indexing) back as dense matrices
    [parts, 32 MT, n_cols] (parts: hi, lo' for precision 3) of fp16 BITS; col_of(half, slot) -> column or -1 (must then be packed as 0)"""
    w_off, b_off, QS, MT = [int(v) for v in lay[l]]
    steps, parts = QS // 8, 2 if precision == 3 else 1
    frag = w[w_off * 16:(w_off + MT * steps * parts * 64) * 16].view(np.uint16).reshape(MT, steps, parts, 64, 8)
    out = np.zeros((parts, 32 * MT, n_cols), np.uint16)
    for m in range(MT):
        for s in range(steps):
            for h in range(2):
                for e in range(8):
                    c = col_of(h, 8 * s + e)
                    v = frag[m, s, :, h * 32:(h + 1) * 32, e]      # [parts, 32 rows]
                    if c < 0:
                        assert not (v & 0x7FFF).any(), "a padding slot carries a weight"
                    else:
                        out[:, 32 * m:32 * m + 32, c] = v
    return out


def act_column(h, q):
    """hidden slot (half, q) -> unit: the output value 16 m + r of half h is row (r & 3) + 8 (r >> 2) + 4 h of tile m"""
    m, r = divmod(q, 16)
    return 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h
