"""tests/flip_reference.py -- the float64 restatement of the reference's FLIP (src/util/flip_loss.py:61-105 as src/evaluate.py:120-145
calls it) that the GPU tests hold adanerf_flip against -- is itself held against the reference's own output, committed as
tests/golden/flip_*.npz by tools/gen_flip_golden.py.

Bound: every fixture stores ``ref_fp32_residual`` = max |reference fp32 map - restatement| (and the same for the mean) as the
generator measured it.  The restatement must reproduce the stored reference map within 4 x that figure: a restatement that is right
stays inside 1 x by construction (the margin covers a numpy / libm whose float64 rounds differently from the generator's), a wrong
one -- another filter, a dropped clamp, swapped padding -- is off by orders of magnitude more.  Floor 1e-6 where the stored residual
is an exact 0."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flip_reference as F
from conftest import GOLD, ROOT

FLOOR = 1e-6


@pytest.mark.parametrize("name", F.FIXTURES)
def test_restatement_reproduces_the_reference_map(name):
    z = F.load_fixture(name)
    m = z["meta"]
    assert z["ref_map"].dtype == np.float32 and z["ref_map"].shape == (m["height"], m["width"]) == z["test"].shape[:2]
    assert np.isfinite(z["ref_map"]).all() and (z["test"] < 0).any() and (z["test"] > 1).any()
    assert list(F.radii(z["ppd"])) == m["radii"]
    err = float(np.max(np.abs(z["map64"] - z["ref_map"].astype(np.float64))))
    err_mean = abs(z["mean64"] - float(z["ref_mean"]))
    print("%s: map %.3e (stored %.3e)  mean %.3e (stored %.3e)" % (name, err, m["ref_fp32_residual"], err_mean, m["ref_fp32_residual_mean"]))
    assert err <= max(4 * m["ref_fp32_residual"], FLOOR)
    assert err_mean <= max(4 * m["ref_fp32_residual_mean"], FLOOR)
    # the stored figures are what they claim to be: the rounding error of fp32 arithmetic, not a disagreement about the algorithm
    assert m["ref_fp32_residual"] < 1e-3 and m["ref_fp32_residual_mean"] < 1e-4


def test_fixture_set_covers_the_radii():
    assert F.radii(F.DEFAULT_PPD) == (10, 9) and F.radii(30.0) == (5, 4) and F.radii(140.0) == (19, 18)
    assert sorted(os.path.basename(p)[:-4] for p in os.listdir(GOLD) if p.startswith("flip_")) == sorted(F.FIXTURES)


def test_identical_images_give_an_all_zero_map():
    z = F.load_fixture("flip_97x61")
    for img in (z["test"], z["ref"]):
        mean, m = F.flip(img, img)
        assert mean == 0.0 and not m.any()


def test_symmetric_in_its_arguments():
    for name in ("flip_37x23", "flip_64x48_ppd30"):
        z = F.load_fixture(name)
        mean, m = F.flip(z["ref"], z["test"], z["ppd_arg"])
        assert np.array_equal(m, z["map64"]) and mean == z["mean64"]


def test_nan_stays_within_the_filter_radius():
    z = F.load_fixture("flip_64x48_ppd30")
    t = z["test"].copy()
    t[20, 30, 1] = np.nan
    m = F.flip_map(t, z["ref"], 30.0)
    far = np.maximum(np.abs(np.arange(48)[:, None] - 20), np.abs(np.arange(64)[None, :] - 30)) > 5
    assert np.array_equal(m[far], z["map64"][far]) and np.isnan(m[20, 30]) and np.isnan(np.mean(m))


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is only present in the build container")
def test_committed_fixture_equals_a_fresh_generator_run(tmp_path):
    name = "flip_37x23"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_flip_golden.py"), "--only", name, "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    new, old = np.load(os.path.join(str(tmp_path), name + ".npz")), np.load(os.path.join(GOLD, name + ".npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in new.files:
        if k == "meta":
            assert json.loads(bytes(new[k]).decode()) == json.loads(bytes(old[k]).decode())
        else:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and np.array_equal(new[k], old[k]), k


def test_header_declares_and_library_exports_adanerf_flip():
    import adanerf_amd
    from adanerf_amd import renderer as R
    src = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    assert re.search(r"\bint\s+adanerf_flip\s*\(\s*adanerf_ctx\s*\*", src)
    assert "src/evaluate.py:120-145" in src and "src/util/flip_loss.py" in src
    assert re.search(r"#define\s+ADANERF_ABI_VERSION\s+4\b", src)
    adanerf_amd.build_library()
    lib = R.load_library()
    assert hasattr(lib, "adanerf_flip") and "adanerf_flip" in R.EXPORTS
    assert "k_flip.hip.hpp" in adanerf_amd.build.LIB_DEPS
