"""CPU-only checks of the per-ray sample budgets (adanerf_set_budget_map / adanerf_foveate / adanerf_compact_budget): the property the
feature rests on -- the selection at (n_r <= N, thr_r >= thr) is a trim of the row the selection at (N, thr) wrote -- against the oracle's
select_adaptive; the C ABI declares and exports the three calls; the hosts' --fovea spec and `gaze` script token accept what they should
and nothing else.  What it renders: tests/test_gpu_budget_map.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import budget_reference as B
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def _rows(kind, rng, rows):
    if kind == "uniform":
        return rng.uniform(-0.5, 1.5, (rows, 128)).astype(F32)
    if kind == "quantised":      # multiples of 0.25: ties at every cut
        return (np.round(rng.uniform(-0.5, 1.5, (rows, 128)) * 4) / 4).astype(F32)
    if kind == "nonfinite":
        x = rng.uniform(-0.5, 1.5, (rows, 128)).astype(F32)
        x[rng.random(x.shape) < 0.1] = np.nan
        x[rng.random(x.shape) < 0.05] = np.inf
        x[rng.random(x.shape) < 0.05] = -np.inf
        x[:8] = np.nan
        return x
    x = np.full((rows, 128), -1.0, F32)      # sparse: a few bins carry a value
    for r in range(rows):
        k = rng.integers(0, 6)
        x[r, rng.choice(128, k, replace=False)] = rng.uniform(0.0, 1.5, k)
    return x


@pytest.mark.parametrize("n_max", [1, 2, 4, 8, 16, 32])
def test_the_trim_of_the_wide_selection_is_the_narrow_selection(n_max):
    """12 000 rows in all (4 kinds x 500 rows x 6 N): counts, bins and weight bits of trim(select(N, thr)) equal select(n_r, thr_r) for
    random n_r in 0..N+3 (0 and > N fall back to N) and thr_r drawn from below / at / above the context's threshold, above every value,
    +inf and NaN."""
    rng = np.random.default_rng(1000 + n_max)
    thr = 0.25
    for kind in ("uniform", "quantised", "nonfinite", "sparse"):
        orc = _rows(kind, rng, 500)
        n_map = rng.integers(0, n_max + 4, 500).astype(np.uint8)
        thr_map = rng.choice(np.array([0.1, 0.25, 0.5, 0.75, 1.0, 2.0, np.inf, np.nan], F32), 500)
        n_eff, thr_eff = B.effective(n_map, thr_map, 500, n_max, thr)
        assert n_eff.min() >= 1 and n_eff.max() <= n_max and (thr_eff >= F32(thr)).all()
        got = B.trim(*O.select_adaptive(orc, n_max, thr), n_eff, thr_eff)
        want = B.expected_selection(orc, n_max, thr, n_map, thr_map)
        for g, w, what in zip(got, want, ("counts", "bins", "weights")):
            assert g.tobytes() == w.tobytes(), (kind, n_max, what)
        # and without maps the trim changes nothing
        plain = O.select_adaptive(orc, n_max, thr)
        same = B.trim(*plain, *B.effective(None, None, 500, n_max, thr))
        assert all(a.tobytes() == np.asarray(b, a.dtype).tobytes() for a, b in zip(same, plain)), (kind, n_max)


def test_ring_fill_reference_against_a_direct_distance_test():
    """the integer rule is the Euclidean one: pixel centre (x + 0.5, y + 0.5) within radius R of the gaze, boundary included"""
    rings = [(3, 8, 0.2), (7, 4, 0.3), (2, 0.5)]
    n_map, thr_map = B.ring_fill(21, 13, (10.5, 6.5), rings)
    yy, xx = np.divmod(np.arange(21 * 13), 21)
    d2 = (xx + 0.5 - 10.5) ** 2 + (yy + 0.5 - 6.5) ** 2
    want = np.where(d2 <= 9, 8, np.where(d2 <= 49, 4, 2))
    assert np.array_equal(n_map, want) and np.array_equal(thr_map, np.where(d2 <= 9, F32(0.2), np.where(d2 <= 49, F32(0.3), F32(0.5))))
    assert B.gaze_half_pixels(-20.25) == -40 and B.gaze_half_pixels(0.25) == 0 and B.gaze_half_pixels(0.75) == 2 and B.gaze_half_pixels(1e30) == 2 ** 31
    # shards: the ranks' maps are the whole frame's, strip by strip
    whole = B.ring_fill(21, 13, (4.0, 30.0), rings)[0]
    from adanerf_amd import sharding
    for rank in range(3):
        part = B.ring_fill(21, 13, (4.0, 30.0), rings, strip_rows=4, world=3, rank=rank)[0]
        assert np.array_equal(part, whole[sharding.local_to_pixel(21, 13, 4, 3, rank)])


GOOD_SPECS = [("100:8:0.2,200:4:0.3,2:0.4", [(100, 8, 0.2), (200, 4, 0.3), (2, 0.4)]), ("2:0.5", [(2, 0.5)]), ("0:0:0,255:1e-3", [(0, 0, 0.0), (255, 0.001)]),
              ("1:1:1,2:2:2,3:3:3,4:4:4,5:5:5,6:6:6,7:7:7,8:8:8,9:9", [(k, k, float(k)) for k in range(1, 9)] + [(9, 9.0)]), ("5:4:inf,0:0.2", [(5, 4, float("inf")), (0, 0.2)])]
BAD_SPECS = ["", "8", "100:8:0.2", "100:8:0.2,", "100:8,2:0.4", "200:8:0.2,100:4:0.3,2:0.4", "100:8:0.2,100:4:0.3,2:0.4", "-1:8:0.2,2:0.4",
             "100:256:0.2,2:0.4", "100:8:0.2,-1:0.4", "100:8:nan,2:0.4", "100:8:0.2,2:abc", "1.5:8:0.2,2:0.4", "100:8:0.2:1,2:0.4",
             "1:1:1,2:2:2,3:3:3,4:4:4,5:5:5,6:6:6,7:7:7,8:8:8,9:9:9,10:10"]


def test_fovea_spec_parsing_python_and_cli(lib, tmp_path):
    for spec, want in GOOD_SPECS:
        assert R.parse_fovea(spec) == want, spec
    for spec in BAD_SPECS:
        with pytest.raises(ValueError):
            R.parse_fovea(spec)
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).fovea is None
    assert ap.parse_args(["m", "d", "--fovea", "100:8:0.2,2:0.4"]).fovea == [(100, 8, 0.2), (2, 0.4)]
    with pytest.raises(SystemExit):
        ap.parse_args(["m", "d", "--fovea", "100:8:0.2"])
    import inspect
    assert inspect.signature(E.evaluate).parameters["fovea"].default is None
    exe = _replay_exe(tmp_path)
    out = subprocess.run([exe, "--fovea"] + [s for s, _ in GOOD_SPECS] + BAD_SPECS, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(GOOD_SPECS) + len(BAD_SPECS)
    for (spec, want), g in zip(GOOD_SPECS, got):
        f = g.split()
        assert f[0] == "ok" and f[1] == "rings=%d" % (len(want) - 1), (spec, g)
        parsed = [tuple(int(v) for v in e.split(":")[:-1]) + (F32(e.split(":")[-1]),) for e in f[2:]]      # the host keeps thresholds as float
        assert parsed == [tuple(e[:-1]) + (F32(e[-1]),) for e in want], (spec, g)
    for spec, g in zip(BAD_SPECS, got[len(GOOD_SPECS):]):
        assert g.split()[0] == "bad", (spec, g)
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--fovea R:N:T[,R:N:T...],N:T" in usage and "gaze <X> <Y>" in usage
    bad = subprocess.run([cli, "model", "--fovea", "200:8:0.2,100:4:0.3,2:0.4", "--dry-run"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "strictly ascending" in bad.stdout


def test_header_declares_and_library_exports_the_budget_calls(lib, tmp_path):
    """A C99 translation unit that takes the address of the three calls with their exact prototypes compiles against include/adanerf_hip.h
    (-Wall -Werror -pedantic) and links against the library; the ABI version is still 4; the ctypes host binds them."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "budget_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "budget_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "set_budget_map(NULL) rc=-1 foveate(NULL) rc=-1 compact_budget(NULL) rc=-1 abi=4"
    for name in ("adanerf_set_budget_map", "adanerf_foveate", "adanerf_compact_budget"):
        assert name in R.EXPORTS and hasattr(lib, name)
    assert lib.adanerf_set_budget_map(None, None, None) == -1          # ADANERF_EINVAL: no context
    syms = subprocess.run(["nm", "-D", "--defined-only", adanerf_amd.library_path()], capture_output=True, text=True, check=True).stdout
    assert all(" T %s\n" % name in syms for name in ("adanerf_set_budget_map", "adanerf_foveate", "adanerf_compact_budget"))
    for name in ("set_budget_map", "foveate", "foveate_device", "compact_budget", "budget_buffers"):
        assert name in dir(R.NeuralRenderer)


def _replay_exe(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to build the replay check"
    from adanerf_amd.build import HOST, LIBDIR
    srcs = [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".cpp") and f != "main.cpp"]
    exe = str(tmp_path / "replay_gaze_token_check")
    if not os.path.exists(exe):
        subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "replay_gaze_token_check.cpp")] + srcs +
                       ["-L", LIBDIR, "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


LINES = [
    # (script line, parses, gaze x, gaze y, size pending, selection pending)
    ("gaze 400.5 300", True, 400.5, 300.0, False, False),
    ("gaze -20.25 10", True, -20.25, 10.0, False, False),
    ("gaze 1e6 -1e6 n 4", True, 1e6, -1e6, False, True),
    ("+w gaze 1 2 size 40 30 -w", True, 1.0, 2.0, True, False),
    ("gaze 1 2 gaze 3 4", True, 3.0, 4.0, False, False),       # the last one holds
    ("n 4", True, 0.0, 0.0, False, True),                      # no gaze token: the frame centre stays in charge
    ("gaze", False, 0.0, 0.0, False, False),
    ("gaze 5", False, 0.0, 0.0, False, False),
    ("gaze 5 abc", False, 0.0, 0.0, False, False),
    ("gaze nan 5", False, 0.0, 0.0, False, False),
    ("gaze 5 inf", False, 0.0, 0.0, False, False),
    ("gaze 5x 5", False, 0.0, 0.0, False, False),
    ("gaze 5 6 7", False, 5.0, 6.0, False, False),             # refused at the stray word; the host stops at a malformed line
]


def test_script_grammar_accepts_and_rejects_the_gaze_token(lib, tmp_path):
    """InputHandler::replay through a stand-alone program over the host's own sources: `gaze <X> <Y>` reaches NeuralRenderer::setGaze next to
    the other events of the line; a missing, malformed or non-finite value and a stray word make the line malformed."""
    exe = _replay_exe(tmp_path)
    out = subprocess.run([exe] + [ln for ln, *_ in LINES], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(LINES)
    for (line, ok, gx, gy, size_p, sel_p), g in zip(LINES, got):
        f = dict(kv.split("=") for kv in g.split()[1:])
        assert g.split()[0] == ("ok" if ok else "bad"), (line, g)
        assert int(f["start"]) == 1 and (float(f["gx"]), float(f["gy"])) == (gx, gy), (line, g)
        assert (int(f["size_pending"]), int(f["sel_pending"])) == (int(size_p), int(sel_p)), (line, g)


def test_cli_dry_run_replays_gaze_tokens(lib, tmp_path):
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    cli = adanerf_amd.build.build_cli()
    good = tmp_path / "good.txt"
    good.write_text("+w\ngaze 4 3\n-w gaze 20 -5 size 12 10\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--fovea", "4:8:0.2,2:0.4", "--script", str(good), "--dry-run", "--log-camera"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("camera ")]) == 3, out.stdout + out.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("+w\ngaze 4\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(bad), "--dry-run"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "malformed script line 2: gaze 4" in out.stdout
