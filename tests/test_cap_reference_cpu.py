"""CPU-only checks of the sample cap's numpy reference (tests/cap_reference.py): the brute-force rule against a second, independent
statement (sort all entries, walk the thresholds downward, count), on random and built rows; and a proof that the built rows discriminate:
each of four plausible wrong rules gives another answer on at least one of them.  Also the C ABI's declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import cap_reference as K

import adanerf_amd
from adanerf_amd import renderer as R

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the second statement -----------------------------------------------------------------------------------------------------------------

def walk_threshold(count, wts, cap_total):
    """t* by one walk: every live non-NaN entry sorted by value, largest first; going down, a group of equal values joins at a time and the
    running T = sum over non-empty rows of max(1, entries joined so far) is kept in integers.  The last value at which T still fits is t*."""
    count = np.asarray(count).astype(np.int64)
    if int(count.sum()) <= cap_total:
        return None
    entries = []
    for r in range(len(count)):
        for k in range(int(count[r])):
            v = float(wts[r, k])
            if v == v:
                entries.append((v + 0.0 if v != 0 else 0.0, r))
    entries.sort(key=lambda e: -e[0])
    joined = np.zeros(len(count), np.int64)
    total = int((count > 0).sum())      # T(+inf side): every non-empty row keeps one
    best = None
    i = 0
    while i < len(entries):
        v = entries[i][0]
        while i < len(entries) and entries[i][0] == v:
            r = entries[i][1]
            if joined[r] >= 1:
                total += 1
            joined[r] += 1
            i += 1
        if total <= cap_total:
            best = v
        else:
            break
    return F32(best) if best is not None else K.INF


def walk_apply(count, bins, wts, cap_total):
    """the trim, restated without the budget reference: per row the entries >= t*, else the first of (value descending, bin ascending)"""
    t = walk_threshold(count, wts, cap_total)
    count = np.asarray(count).astype(np.int32).copy()
    if t is None:
        return -K.INF, count, bins, wts
    ob, ow = np.full_like(bins, -1), np.zeros_like(wts)
    for r in range(len(count)):
        c = int(count[r])
        ks = [k for k in range(c) if wts[r, k] >= t]
        if not ks and c > 0:
            best = 0
            for k in range(1, c):
                if wts[r, k] > wts[r, best]:
                    best = k
            ks = [best]
        count[r] = len(ks)
        ob[r, :len(ks)], ow[r, :len(ks)] = bins[r, ks], wts[r, ks]
    return t, count, ob, ow


def same_selection(a, b):
    (ta, ca, ba, wa), (tb, cb, bb, wb) = a, b
    return F32(ta).tobytes() == F32(tb).tobytes() and ca.tobytes() == cb.tobytes() and ba.tobytes() == bb.tobytes() and wa.tobytes() == wb.tobytes()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (orc, n_max, thr, cap) in K.built_cases().items():
        out[name] = (K.selection(orc, n_max, thr), cap)
    for n, n_max in ((1, 8), (33, 8), (257, 16), (257, 24), (700, 8)):
        orc, n_max, thr, cap = K.random_case(n, n_max)
        out["random_%d_%d" % (n, n_max)] = (K.selection(orc, n_max, thr), cap)
    return out


def test_the_two_statements_agree(cases):
    for name, ((cnt, bins, wts), cap) in cases.items():
        assert cap >= len(cnt), name
        a, b = K.apply(cnt, bins, wts, cap), walk_apply(cnt, bins, wts, cap)
        assert same_selection(a, b), name
        t, c2 = a[0], a[1]
        assert int(c2.sum()) <= max(cap, int(cnt.sum()) if t == -K.INF else cap), name
        if t != -K.INF:
            assert int(c2.sum()) <= cap and int(c2.sum()) == K.kept_total(cnt, wts, t), name
            assert t >= F32(K.THR), name      # a fallback value below the threshold is never t*


def test_rows_emptied_by_a_depth_limit_count_nothing(cases):
    (cnt, bins, wts), _ = cases["random_257_16"]
    cnt = cnt.copy()
    cnt[::3] = 0
    cap = max(257, int(0.6 * cnt.sum()))
    a, b = K.apply(cnt, bins, wts, cap), walk_apply(cnt, bins, wts, cap)
    assert same_selection(a, b) and (a[1][::3] == 0).all() and a[1].sum() <= cap and a[0] > 0


def test_what_the_built_rows_are_for(cases):
    """each built case does what its name says"""
    def t_of(name):
        (cnt, bins, wts), cap = cases[name]
        return K.apply(cnt, bins, wts, cap)

    n = 600
    t, c, _, _ = t_of("tie_jump")
    assert t == F32(0.9) and c.sum() == n            # well under C = 2.5 n: the tie at 0.5 does not fit
    t, c, _, _ = t_of("tie_fits")
    assert t == F32(0.5) and c.sum() == 3 * n
    t, c, b, _ = t_of("all_equal")
    assert t == K.INF and (c == 1).all() and (b[:, 0] == 3).all()
    for name in ("low10", "mid11", "top11"):
        t, c, _, _ = t_of(name)
        (cnt, _, wts), cap = cases[name]
        assert np.isfinite(t) and 257 < c.sum() <= cap < cnt.sum()
        assert len(K.present_values(cnt, wts)) > (10 if name == "top11" else 100)
    t, c, _, _ = t_of("fallback_rows")
    assert t >= F32(K.THR) and (c >= 1).all()
    assert t_of("inf_present")[0] == K.INF and t_of("inf_present")[1].sum() == 300
    assert t_of("inf_above")[0] == F32(0.7)
    t, c, _, w = t_of("nan_fallback")
    assert np.isnan(w[::4, 0]).all() and (c[::4] == 1).all() and c.sum() <= 500
    assert (t_of("c_is_n")[1] == 1).all()
    assert t_of("c_is_t_now")[0] == -K.INF and t_of("c_above_t_now")[0] == -K.INF
    (cnt, _, _), cap = cases["c_is_t_now_minus_1"]
    t, c, _, _ = t_of("c_is_t_now_minus_1")
    assert t != -K.INF and c.sum() < cnt.sum()


# ---- wrong rules: each must be told apart by at least one built case ----------------------------------------------------------------------

def _kept(count, wts, t, strict=False, count_fallback=True):
    count = np.asarray(count).astype(np.int64)
    live = np.arange(wts.shape[1])[None, :] < count[:, None]
    with np.errstate(invalid="ignore"):
        a = (((wts > t) if strict else (wts >= t)) & live).sum(axis=1)
    return int(np.where(count == 0, 0, np.maximum(1, a) if count_fallback else a).sum())


def wrong_largest(count, wts, cap):
    """the largest t that fits instead of the smallest"""
    if int(count.sum()) <= cap:
        return None
    fits = [v for v in K.present_values(count, wts) if _kept(count, wts, v) <= cap]
    return F32(max(fits)) if fits else K.INF


def wrong_strict(count, wts, cap):
    """> instead of >= when counting"""
    if int(count.sum()) <= cap:
        return None
    fits = [v for v in K.present_values(count, wts) if _kept(count, wts, v, strict=True) <= cap]
    return F32(min(fits)) if fits else K.INF


def wrong_no_fallback(count, wts, cap):
    """the entry a row keeps when nothing reaches t is not counted"""
    if int(count.sum()) <= cap:
        return None
    fits = [v for v in K.present_values(count, wts) if _kept(count, wts, v, count_fallback=False) <= cap]
    return F32(min(fits)) if fits else K.INF


def wrong_split_ties(count, wts, cap):
    """ties split: the threshold one value below t*, on the grounds that part of the tie would still fit"""
    t = K.threshold(count, wts, cap)
    if t is None:
        return None
    vals = K.present_values(count, wts)
    below = vals[vals < t]
    return F32(below.max()) if len(below) and _kept(count, wts, t) < cap else t


@pytest.mark.parametrize("wrong", [wrong_largest, wrong_strict, wrong_no_fallback, wrong_split_ties], ids=lambda f: f.__name__)
def test_a_wrong_rule_is_rejected_by_the_built_rows(cases, wrong):
    rejected = []
    for name, ((cnt, bins, wts), cap) in cases.items():
        if name.startswith("random"):
            continue
        right, got = K.threshold(cnt, wts, cap), wrong(cnt, wts, cap)
        if (right is None) != (got is None) or (right is not None and F32(right).tobytes() != F32(got).tobytes()):
            rejected.append(name)
    assert rejected, "no built case tells %s from the rule" % wrong.__name__


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------

NAMES = ("adanerf_set_sample_cap", "adanerf_sample_cap_report", "adanerf_compact_cap")


def test_entry_points_are_declared_exported_and_refuse_a_null_context():
    adanerf_amd.build_library()
    lib = R.load_library()
    src = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n) and n in R.EXPORTS
    m = re.search(r"typedef struct adanerf_cap_report \{(.*?)\} adanerf_cap_report;", src, re.S)
    assert m and [f.split()[-1] for f in m.group(1).strip().rstrip(";").split(";")] == [f[0] for f in R.CapReport._fields_]
    assert C.sizeof(R.CapReport) == 24
    rep = R.CapReport()
    assert lib.adanerf_set_sample_cap(None, 2.0) == -1 and lib.adanerf_sample_cap_report(None, C.byref(rep)) == -1
    assert lib.adanerf_compact_cap(None, None, 0, 8, 0.25, None, None, None, None, None, None, 0, None, None, None, None, None, None) == -1


def test_cli_takes_a_sample_cap_and_replays_cap_tokens(tmp_path):
    """--sample-cap X and the script token `cap X`, without a device (--dry-run): what the library would refuse is refused by the host"""
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--sample-cap X" in usage and "cap <X>" in usage
    good = tmp_path / "good.txt"
    good.write_text("+w\ncap 4.5\n-w cap 0\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--sample-cap", "6", "--script", str(good), "--dry-run", "--log-camera"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("camera ")]) == 3, out.stdout + out.stderr
    for bad_line in ("cap", "cap 0.5", "cap nan", "cap inf", "cap 4x"):
        bad = tmp_path / "bad.txt"
        bad.write_text("+w\n%s\n" % bad_line)
        out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(bad), "--dry-run"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "malformed script line 2" in out.stdout, (bad_line, out.stdout)
    for args in (["--sample-cap", "0.5"], ["--sample-cap", "nan"], ["--sample-cap", "4", "--fovea-density", "4:1,2"], ["--sample-cap", "4", "--oracle"]):
        out = subprocess.run([cli, md, "-s", "16", "12", "--dry-run"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--sample-cap" in out.stdout, (args, out.stdout)
