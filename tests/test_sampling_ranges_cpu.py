"""The range probes of tests/range_networks.py, CPU side: what tests/test_gpu_sampling_ranges.py relies on is shown here on the oracle's
features of the 97 x 61 frame of synthetic_fixed8's camera --

 a. the per-layer predictions equal mlp_reference.sampling_mlp64 under "split" / "fp16" / "exact", rounded to fp32, bit for bit on the
    constants table and on the ray-driven rows (inside the one-rounding bracket where the cross term has two non-zero products); a ray the
    prediction calls BAD is non-finite in every column of the reference's row;
 b. which table entries the model itself sends out of range: nextafter(65520, 0) in the split engine (hi = 65504, lo' = 32768: the value
    65520, inf at the next hidden layer), nothing else below 65520;
 c. the class floors (range_networks.FLOORS) on that frame: conditions on the construction, not measurements;
 d. every emulated wrong kernel (range_networks.FAULTS) changes named table entries and ray-driven rows (REJECTS);
 e. adanerf_host_pack_weights (split pairs and plain fp16) puts exactly split_parts / astype(float16) of every weight of a range probe at the
    places mfma_emulation reads, the subnormal, zero-hi and 2^-37 gains included; a weight >= 65520 packs as hi = inf, lo' = -inf (the
    network adanerf_create refuses outside ADANERF_SAMPLING_FP32)."""
import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
import probe_networks as P
import range_networks as RN
import tie_networks as T
from conftest import load_case
from mfma_emulation import pack_weights

import adanerf_amd
from adanerf_amd import renderer as R

MODEL = {"split": "split", "fp16": "fp16", "fp32": "exact"}
# (depth, width): the fixed kernels' topology (tile 7 of every hidden layer is the pending tile) and a run-time-shaped one that needs chunks
TOPOLOGIES = [(8, 256), (4, 64)]


@pytest.fixture(scope="module")
def frame():
    z, meta, sc = load_case("synthetic_fixed8")
    feat = P.frame_inputs(sc, z["pose"], z["rot"])[3]
    feat.setflags(write=False)
    return sc, feat


def probe_sets(sc, feat):
    """name -> entries, as the GPU test builds them"""
    dc, pc = T.identity_columns(sc)
    sets = dict(table=RN.table_entries(), top=RN.const_entries(RN.TOP), top_split=RN.const_entries(RN.TOP_SPLIT),
                overflow=RN.const_entries(RN.OVERFLOW), overflow_finite32=RN.const_entries(RN.OVERFLOW_FINITE32), rays=RN.ray_entries(dc, pc, feat))
    for i, e in enumerate(RN.edge_probes(dc[:2], feat)):
        sets["edge%d" % i] = e
    return sets


@pytest.mark.parametrize("depth,width", TOPOLOGIES)
def test_predictions_equal_the_reference(frame, depth, width):
    sc, feat = frame
    seen = {}
    for name, entries in probe_sets(sc, feat).items():
        for ci, ent in enumerate(RN.chunks(entries, width)):
            net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=ci)
            if width == 256:
                assert all(0 in t and 7 in t for t in RN.tiles_visited(chains, width)), "a hidden layer without a unit in tile 0 or in the pending tile"
            for engine, model in MODEL.items():
                lo, hi, rne, bad = RN.bracket(feat, chains, engine)
                with np.errstate(over="ignore", invalid="ignore"):
                    y = M.sampling_mlp64(feat, net, model).astype(np.float32)
                c = RN.compare(y[:, :len(ent)], lo, hi, rne, bad)
                assert not c["wrong"].any(), (name, ci, engine, [ent[j][0] for j in np.flatnonzero(c["wrong"].any(axis=0))])
                assert not y[~bad][:, len(ent):].any()
                assert not np.isfinite(y[bad]).any(), (name, engine, "a BAD ray with a finite column")
                s = seen.setdefault((name, engine), dict(bad=0, rays=0, by_bracket=0))
                s["bad"] += c["bad_rays"]
                s["rays"] += feat.shape[0]
                s["by_bracket"] += c["by_bracket"]
    n = feat.shape[0]
    every = lambda k: seen[k]["bad"] == seen[k]["rays"]
    none = lambda k: seen[k]["bad"] == 0
    # b: what is finite and what is not, per engine
    for engine in MODEL:
        assert none(("table", engine)) and none(("rays", engine)) and none(("top_split", engine)), engine
        assert every(("overflow", engine)), engine      # +inf and NaN: no matrix product carries them, fp32 included
    assert every(("top", "split")) and none(("top", "fp16")) and none(("top", "fp32"))      # nextafter(65520, 0): the split engine alone
    assert every(("overflow_finite32", "split")) and every(("overflow_finite32", "fp16")) and none(("overflow_finite32", "fp32"))
    for e in ("edge0", "edge1"):      # the edge crosses the frame: both kinds of ray, in both 16-bit engines; all finite in fp32
        assert 0.2 * n < seen[e, "split"]["bad"] < 0.9 * n and 0.2 * n < seen[e, "fp16"]["bad"] < 0.9 * n and none((e, "fp32")), (e, seen[e, "split"])


def test_the_table_entry_beyond_the_split_range(frame):
    """nextafter(65520, 0) alone is what the split engine loses below 65520, and only behind a second hidden layer; 65520 - 2^-7 stays"""
    sc, feat = frame
    for (name, v), want in zip(RN.TOP + RN.TOP_SPLIT[3:], [False, False, False, True, False]):
        net, chains = RN.range_probe(sc.n_in0, 4, 64, RN.const_entries([(name, v)]))
        out, bad = RN.predict(feat[:1], chains, "split")
        assert bool(bad[0]) == want, name
        if not want:
            assert out[0, 0] == np.float32(v)
    hi, lo = M.split_parts(RN.LAST_BELOW_EDGE)
    assert (hi, lo) == (65504.0, 32768.0) and hi + lo / M.SPLIT == float(RN.F16_EDGE)
    hi, lo = M.split_parts(np.float32(RN.TOP_SPLIT[3][1]))
    assert (hi, lo) == (65504.0, 32752.0)


def test_class_floors(frame):
    sc, feat = frame
    dc, pc = T.identity_columns(sc)
    for depth, width in TOPOLOGIES:
        flags = [RN.class_flags(feat, RN.range_probe(sc.n_in0, depth, width, ent, seed=ci)[1])
                 for ci, ent in enumerate(RN.chunks(RN.ray_entries(dc, pc, feat), width))]
        RN.check_floors(RN.class_shares(flags), "oracle features %dx%d" % (depth, width))


# fault -> engine -> the table entries it must change.  A truncated hi is absorbed by lo' in the split engine on every finite table entry (lo'
# takes the other sign and the sum is the same 22 bits): there 65520 shows it (it stays finite), the ray-driven rows, and the plain-fp16 table.
REJECTS = {
    "ftz": dict(split=["1e-5", "2^-26", "1e-8", "2^-35", "2^-36+2^-50", "0.75 x 2^-30"], fp16=["2^-14-2^-24", "2^-24", "3*2^-25", "0.75 x 2^-20"]),
    "rtz_hi": dict(split=["65520"], fp16=["1+3*2^-11", "1+2^-11+2^-23", "3*2^-25"]),
    "rtz_lo": dict(split=["1+2^-11+2^-23", "1+2^-11-2^-23", "2^-25+2^-40", "2^-36+2^-50"]),
    "double_lo": dict(split=["1e-5", "2^-36+2^-50"]),
    "saturate": dict(split=["65520", "1e5"], fp16=["65520", "1e5", "3e38"]),
    "no_cross": dict(split=["1+2^-11", "1+2^-22", "1+2^-23", "2^-25", "2^-35", "65512"]),
    "no_wlo": dict(split=["0.75 x 2^-30", "0.75 x 1/3", "0.75 x pi", "0.75 x 65000", "(1+2^-22) x 1/3"]),
    "relu_nan0": dict(split=["nan"], fp16=["nan"]),
}


# plain fp16: an overflowed chain stays inf by itself, and the NaN a faulty ReLU would drop arises in the OTHER units (0 x inf), which the
# per-chain prediction does not follow -- on the device the probe's idle columns would come back finite, which the GPU test's "every column of
# a BAD ray is non-finite" rejects
NO_RAY_ROWS = {("relu_nan0", "fp16")}


def outcome(sc, feat1, entry, engine, fault):
    net, chains = RN.range_probe(sc.n_in0, 4, 64, [entry])
    out, bad = RN.predict(feat1, chains, engine, fault=fault)
    return ("bad",) if bad[0] else ("bits", int(RN.bits(out)[0, 0]))


@pytest.mark.parametrize("fault", RN.FAULTS)
def test_emulated_wrong_kernels_are_rejected(frame, fault):
    sc, feat = frame
    assert set(REJECTS) == set(RN.FAULTS)
    dc, pc = T.identity_columns(sc)
    table = RN.table_entries() + RN.const_entries(RN.TOP_SPLIT + RN.OVERFLOW)
    ray_sets = [RN.ray_entries(dc, pc, feat)] + RN.edge_probes(dc[:2], feat)
    for engine, names in REJECTS[fault].items():
        changed = [n for n, s in table if outcome(sc, feat[:1], (n, s), engine, fault) != outcome(sc, feat[:1], (n, s), engine, None)]
        assert set(names) <= set(changed), (fault, engine, "named entries the fault leaves alone", sorted(set(names) - set(changed)))
        rows = 0
        for ent in ray_sets:
            net, chains = RN.range_probe(sc.n_in0, 8, 256, ent)
            a, bad_a = RN.predict(feat, chains, engine)
            b, bad_b = RN.predict(feat, chains, engine, fault=fault)
            rows += int(((bad_a != bad_b) | (~bad_a & ~bad_b & (RN.bits(a) != RN.bits(b)).any(axis=1))).sum())
        assert rows >= 1 or (fault, engine) in NO_RAY_ROWS, (fault, engine, "no ray-driven row changes")


# ---- e: the packer ------------------------------------------------------------------------------------------------------------------------

def packed_against_the_rule(lib, d, net, sc, depth, width, prec):
    w, b, lay = pack_weights(lib, d, 0, prec)
    fp, fd = sc.pos_enc[0]
    cols0 = RN.slot_columns_layer0(fp, fd)
    checked = 0
    for l in range(depth):
        wt = np.asarray(net["layers.%d.weight" % l], np.float32)
        n_cols = wt.shape[1]
        dense = RN.dense_weights(w, lay, l, prec, n_cols, (lambda h, q: cols0[h, q]) if l == 0 else
                                 (lambda h, q: RN.act_column(h, q) if RN.act_column(h, q) < n_cols else -1))
        with np.errstate(over="ignore", invalid="ignore"):
            if prec == 3:
                hi, lo = M.split_parts(wt)
                want = [hi.astype(np.float16), lo.astype(np.float16)]
            else:
                want = [wt.astype(np.float16)]
        for part, wp in enumerate(want):
            got = dense[part, :wt.shape[0]]
            assert np.array_equal(got, wp.view(np.uint16)), (l, part, prec)
            assert not (dense[part, wt.shape[0]:] & 0x7FFF).any()      # rows the network does not have
            checked += int((wt != 0).sum())
    return checked


@pytest.mark.parametrize("depth,width,precs", [(8, 256, (3, 1)), (4, 64, (3,)), (5, 128, (3,))])
def test_packer_follows_the_split_rule_on_range_probes(frame, tmp_path, depth, width, precs):
    sc, feat = frame
    adanerf_amd.build_library()
    lib = R.load_library()
    filler = O.synthetic_weights(1).net1
    sets = probe_sets(sc, feat)
    for name in ("table", "rays", "edge1"):
        for ci, ent in enumerate(RN.chunks(sets[name], width)):
            net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=ci)
            d = str(tmp_path / ("%s_%d_%d" % (name, width, ci)))
            O.write_model_dir(d, sc, O.Weights(net, filler))
            for prec in precs:
                assert packed_against_the_rule(lib, d, net, sc, depth, width, prec) >= len(ent)
    # the gains the rule sends to special places
    for g, (hi, lo) in {2.0 ** -20: (2.0 ** -20, 0.0), 2.0 ** -30: (0.0, 2.0 ** -19), 2.0 ** -37: (0.0, 0.0)}.items():
        assert M.split_parts(np.float32(g)) == (hi, lo)


def test_packer_on_a_weight_outside_the_fp16_range(frame, tmp_path):
    """what adanerf_host_pack_weights does today with |w| >= 65520: hi = inf and lo' = -inf, the rule's own answer (adanerf_create refuses
    the network for the 16-bit engines: tests/test_gpu_sampling_ranges.py)"""
    sc, feat = frame
    adanerf_amd.build_library()
    lib = R.load_library()
    for name, g in RN.GAIN_OVER:
        net, chains = RN.range_probe(sc.n_in0, 8, 256, [(name, ("ray", 0, g))])
        d = str(tmp_path / ("over_" + name))
        O.write_model_dir(d, sc, O.Weights(net, O.synthetic_weights(1).net1))
        for prec in (3, 1):
            assert packed_against_the_rule(lib, d, net, sc, 8, 256, prec) >= 2
        with np.errstate(over="ignore"):
            hi, lo = M.split_parts(np.float32(g))
        assert hi == np.inf and lo == -np.inf
