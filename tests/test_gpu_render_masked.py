"""adanerf_render_masked on the GPU.  Every case renders the full frame once into A (rgba8, rgb, depth, acc, disp), pre-fills B with canary
patterns (64 canary elements either side of every buffer), calls the masked render into B and requires
B == mask_reference.expected(canary, A, mask, values) byte for byte in all five outputs, the canaries intact, the mask unmodified and the
list the call built (ADANERF_BUF_RAY_LIST / _COUNT) equal to mask_reference.list_of.  Fixture classroom_n8_thr02, bf16 shading, at 48 x 40
(1920 rays, 15 tiles of 128) and 37 x 29 (1073 rays, ragged everywhere).  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C

import numpy as np
import pytest

import adanerf_oracle as O
import mask_reference as MR
import reproject_reference as RR
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64
SIZES = [(48, 40), (37, 29)]
# per output: elements per pixel, dtype, the canary element
OUTPUTS = [("rgba8", 4, np.uint8, 0xA5), ("rgb", 3, np.float32, np.float32(-1234.5)), ("depth", 1, np.float32, np.float32(-77.25)),
           ("acc", 1, np.float32, np.float32(-3.5)), ("disp", 1, np.float32, np.float32(-9.75))]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("masked_" + name))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _model(tmp_path_factory, "classroom_n8_thr02")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Images:
    """five canaried device images of n pixels, in OUTPUTS' order"""

    def __init__(self, r, n):
        self.r, self.n = r, n
        self.dev = []
        for _, k, dt, canary in OUTPUTS:
            self.dev.append(R.DeviceArray(r, ((PAD + n + PAD) * k,), dt))
        self.fill()

    def fill(self):
        for d, (_, k, dt, canary) in zip(self.dev, OUTPUTS):
            d.upload(np.full((PAD + self.n + PAD) * k, canary, dt))

    def ptr(self, i):
        _, k, dt, _ = OUTPUTS[i]
        return self.dev[i].ptr + PAD * k * np.dtype(dt).itemsize

    def install_aux(self, depth=True, acc=True, disp=True):
        self.r._check(self.r.lib.adanerf_set_aux_outputs(self.r.handle, self.ptr(2) if depth else None, self.ptr(3) if acc else None))
        self.r._check(self.r.lib.adanerf_set_disp_output(self.r.handle, self.ptr(4) if disp else None))

    def get(self):
        """the five images [n, k] after a sync, canaries checked"""
        self.r.sync()
        out = []
        for d, (name, k, dt, canary) in zip(self.dev, OUTPUTS):
            a = d.numpy()
            assert np.all(a[:PAD * k] == canary) and np.all(a[(PAD + self.n) * k:] == canary), "wrote outside the %s output" % name
            out.append(a[PAD * k:(PAD + self.n) * k].reshape(self.n, k))
        return out

    def canaries(self):
        return [np.full((self.n, k), canary, dt) for _, k, dt, canary in OUTPUTS]

    def free(self):
        for d in self.dev:
            d.free()


def full_frame(r, n):
    """A: adanerf_render of the whole frame with every output installed -> (five images, per-ray counts, stats)"""
    a = Images(r, n)
    try:
        a.install_aux()
        st = R.Stats()
        r._check(r.lib.adanerf_render(r.handle, a.ptr(0), a.ptr(1), C.byref(st)))
        imgs = a.get()
        counts = r.buffer(R.BUF_RAY_COUNTS, np.int32, (n,)) if r.info.batch_rays >= n else None
        return imgs, counts, st
    finally:
        r.set_aux_outputs(None, None)
        r.set_disp_output(None)
        a.free()


def masked(r, b, d_mask, values, rgba8=True, rgb=True, stats=True, mask_ptr=True):
    """the C ABI itself -> (rc, n_rendered, stats)"""
    st, m = R.Stats(), C.c_int32(-7)
    rc = r.lib.adanerf_render_masked(r.handle, d_mask.ptr if mask_ptr else None, int(values) & 0xFFFFFFFF, b.ptr(0) if rgba8 else None,
                                     b.ptr(1) if rgb else None, C.byref(st) if stats else None, C.byref(m))
    return rc, m.value, st


def check_case(r, A, mask, values, counts=None, rgba8=True, rgb=True, aux=(True, True, True), tag=""):
    """one masked call into fresh canaries against frame A; returns (the five images, n_rendered, stats)"""
    n = len(mask)
    b = Images(r, n)
    d_mask = R.DeviceArray(r, (n,), np.uint8).upload(mask)
    try:
        b.install_aux(*aux)
        rc, m, st = masked(r, b, d_mask, values, rgba8=rgba8, rgb=rgb)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        got = b.get()
        want_list = MR.list_of(mask, values)
        written = [rgba8, rgb] + list(aux)
        for g, a, c, on, (name, _, _, _) in zip(got, A, b.canaries(), written, OUTPUTS):
            want = MR.expected(c, a, mask, values) if on else c
            diff = int(np.count_nonzero(np.any(bits(g) != bits(want), axis=1)))
            print("%s %s: %d of %d pixels differ (M = %d)" % (tag, name, diff, n, len(want_list)))
            assert diff == 0, (tag, name)
        assert np.array_equal(d_mask.numpy(), mask), "mask modified"
        assert m == len(want_list) and st.rays == m
        assert r.buffer(R.BUF_RAY_LIST_COUNT, np.int32, (1,))[0] == m
        assert np.array_equal(r.buffer(R.BUF_RAY_LIST, np.int32, (m,)), want_list), tag
        if counts is not None:
            assert st.total_samples == int(counts[want_list].sum()), tag
        return got, m, st
    finally:
        r.set_aux_outputs(None, None)
        r.set_disp_output(None)
        d_mask.free()
        b.free()


@pytest.fixture(scope="module")
def ctx(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 48, 40)) as r:
        r.set_camera(z["pose"], z["rot"])
        yield r


@pytest.fixture(scope="module")
def frames(ctx):
    """A per size, rendered once and left unchanged"""
    out = {}
    for w, h in SIZES:
        ctx.set_frame_size(w, h)
        out[(w, h)] = full_frame(ctx, w * h)
        assert len(np.unique(out[(w, h)][0][0][:, :3])) > 16
    return out


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(MR.MASKS))
def test_masked_pixels_equal_the_full_frame(ctx, frames, w, h, name):
    ctx.set_frame_size(w, h)
    A, counts, st_full = frames[(w, h)]
    mask, values = MR.MASKS[name](w * h, w)
    got, m, st = check_case(ctx, A, mask, values, counts, tag="%dx%d %s" % (w, h, name))
    if name == "all":      # the whole frame through the list equals adanerf_render whole
        assert m == w * h and st.total_samples == st_full.total_samples
        for g, a in zip(got, A):
            assert np.array_equal(bits(g), bits(a))


def test_nothing_selected_writes_nothing(ctx, frames):
    w, h = SIZES[1]
    ctx.set_frame_size(w, h)
    for mask, values in ((np.ones(w * h, np.uint8), 1), (np.full(w * h, 32, np.uint8), 0xFFFFFFFF), (np.full(w * h, 255, np.uint8), 0xFFFFFFFF),
                         (np.zeros(w * h, np.uint8), 1 << 31)):
        got, m, st = check_case(ctx, frames[(w, h)][0], mask, values, tag="M=0")
        assert m == 0 and st.rays == 0 and st.total_samples == 0 and st.batches == 0


def test_outputs_are_optional(ctx, frames):
    w, h = SIZES[1]
    ctx.set_frame_size(w, h)
    A, counts, _ = frames[(w, h)]
    mask, values = MR.random30(w * h, w)
    check_case(ctx, A, mask, values, counts, rgb=False, tag="only rgba8")
    check_case(ctx, A, mask, values, counts, rgba8=False, tag="only rgb")
    check_case(ctx, A, mask, values, counts, aux=(False, False, False), tag="no aux maps")
    check_case(ctx, A, mask, values, counts, aux=(False, False, True), tag="disp only")
    check_case(ctx, A, mask, values, counts, aux=(True, False, False), tag="depth only")


def test_two_identical_calls_give_identical_bytes(ctx, frames):
    w, h = SIZES[0]
    ctx.set_frame_size(w, h)
    A, counts, _ = frames[(w, h)]
    mask, values = MR.checkerboard(w * h, w)
    one = check_case(ctx, A, mask, values, counts, tag="first")
    two = check_case(ctx, A, mask, values, counts, tag="second")
    for a, b in zip(one[0], two[0]):
        assert np.array_equal(bits(a), bits(b))
    assert one[1] == two[1] and one[2].total_samples == two[2].total_samples


def test_a_misaligned_mask_pointer(ctx, frames):
    """the 16-byte loads need an aligned mask: one that is not takes the byte path and selects the same pixels"""
    w, h = SIZES[1]
    n = w * h
    ctx.set_frame_size(w, h)
    A = frames[(w, h)][0]
    mask, values = MR.mixed_bytes(n, w)
    b = Images(ctx, n)
    holder = R.DeviceArray(ctx, (n + 16,), np.uint8).upload(np.concatenate([np.zeros(3, np.uint8), mask, np.zeros(13, np.uint8)]))
    try:
        st, m = R.Stats(), C.c_int32(-7)
        assert ctx.lib.adanerf_render_masked(ctx.handle, holder.ptr + 3, values, b.ptr(0), b.ptr(1), C.byref(st), C.byref(m)) == 0
        got = b.get()
        assert m.value == len(MR.list_of(mask, values))
        assert np.array_equal(got[0], MR.expected(b.canaries()[0], A[0], mask, values))
        assert np.array_equal(bits(got[1]), bits(MR.expected(b.canaries()[1], A[1], mask, values)))
    finally:
        holder.free()
        b.free()


def test_chunks_of_batch_rays(model, frames):
    """-bs 256 and M = 700: three chunks, the last partial, against the same frame A"""
    z, sc, d = model
    w, h = SIZES[0]
    mask, values = MR.m_edges(700)(w * h, w)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=256)) as r:
        assert r.info.batch_rays == 256
        r.set_camera(z["pose"], z["rot"])
        got, m, st = check_case(r, frames[(w, h)][0], mask, values, frames[(w, h)][1], tag="bs256 M700")
        assert m == 700 and st.batches == 3


def test_pixel_offset_in_force(ctx):
    w, h = SIZES[1]
    ctx.set_frame_size(w, h)
    ctx.set_pixel_offset(0.25, -0.5)
    try:
        A, counts, _ = full_frame(ctx, w * h)
        check_case(ctx, A, *MR.random30(w * h, w), counts, tag="offset")
    finally:
        ctx.set_pixel_offset(0.0, 0.0)


def test_after_set_selection(model):
    z, sc, d = model
    w, h = SIZES[1]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        r.set_camera(z["pose"], z["rot"])
        r.set_selection(4, 0.3)
        A, counts, _ = full_frame(r, w * h)
        assert counts.max() <= 4
        check_case(r, A, *MR.checkerboard(w * h, w), counts, tag="N4 thr0.3")


def test_buffers_grow_inside_the_masked_call(model, frames):
    """from 16 x 12 up to 48 x 40: the first masked call of the context, at the larger size"""
    z, sc, d = model
    w, h = SIZES[0]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 12)) as r:
        r.set_camera(z["pose"], z["rot"])
        small = full_frame(r, 16 * 12)
        check_case(r, small[0], *MR.checkerboard(16 * 12, 16), small[1], tag="16x12")
        r.set_frame_size(w, h)
        check_case(r, frames[(w, h)][0], *MR.random30(w * h, w), frames[(w, h)][1], tag="grown to 48x40")


def test_guarded_context_renders_the_list_as_the_split_engine(model, frames):
    z, sc, d = model
    w, h = SIZES[0]
    n = w * h
    mask, values = MR.random30(n, w)

    def guarded():
        r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), sampling="guarded", guard_cache=False)
        r.init()
        r.set_camera(z["pose"], z["rot"])
        return r

    # two guarded full renders, without a masked call between them
    r = guarded()
    try:
        f1, _, s1 = full_frame(r, n)
        f2, _, s2 = full_frame(r, n)
    finally:
        r.close()
    r = guarded()
    try:
        g1, _, t1 = full_frame(r, n)
        got, m, st = check_case(r, frames[(w, h)][0], mask, values, frames[(w, h)][1], tag="guarded")      # A: the split context's frame
        assert st.rays_refined == 0
        assert (st.guard_audited, st.guard_violations, st.guard_audit_mismatch, st.guard_widened) == (t1.guard_audited, t1.guard_violations,
                                                                                                      t1.guard_audit_mismatch, t1.guard_widened)
        g2, _, t2 = full_frame(r, n)
    finally:
        r.close()
    print("guard_audited: %d -> %d without the masked call, %d -> %d with it; refined %d / %d and %d / %d" % (
        s1.guard_audited, s2.guard_audited, t1.guard_audited, t2.guard_audited, s1.rays_refined, s2.rays_refined, t1.rays_refined, t2.rays_refined))
    for a, b in zip(f1 + f2, g1 + g2):
        assert np.array_equal(bits(a), bits(b))
    assert (t1.guard_audited, t2.guard_audited) == (s1.guard_audited, s2.guard_audited) and s2.guard_audited > s1.guard_audited > 0
    assert (t1.rays_refined, t2.rays_refined) == (s1.rays_refined, s2.rays_refined)


def _untouched(b):
    got = b.get()
    return all(np.array_equal(bits(g), bits(c)) for g, c in zip(got, b.canaries()))


def test_refused_arguments(ctx, frames):
    w, h = SIZES[1]
    n = w * h
    ctx.set_frame_size(w, h)
    b = Images(ctx, n)
    d_mask = R.DeviceArray(ctx, (n,), np.uint8).upload(np.zeros(n, np.uint8))
    try:
        b.install_aux()
        for kw, word in ((dict(mask_ptr=False), "NULL mask"), (dict(rgba8=False, rgb=False), "both colour outputs NULL"), (dict(values=0), "values == 0")):
            args = dict(values=1)
            args.update(kw)
            rc, m, _ = masked(ctx, b, d_mask, args.pop("values"), **args)
            assert rc == EINVAL and m == -7 and word in ctx.lib.adanerf_last_error(ctx.handle).decode(), kw
            assert _untouched(b), kw
        assert ctx.lib.adanerf_render_masked(None, d_mask.ptr, 1, b.ptr(0), None, None, None) == EINVAL and _untouched(b)
        rc, m, _ = masked(ctx, b, d_mask, 1)
        assert rc == 0 and m == n
    finally:
        ctx.set_aux_outputs(None, None)
        ctx.set_disp_output(None)
        d_mask.free()
        b.free()


UNSUPPORTED = [("dense", "classroom_n8_thr02", dict(num_samples=128, threshold=0.0), "dense"),
               ("pdf", "classroom_pdf_n8", dict(), "PDF"),
               ("coarse_fine", "classroom_coarse_fine_16_24", dict(), "coarse / fine"),
               ("run_time_shaped", "syn_6x128_skip2", dict(), "run-time-shaped"),
               ("sampling_fp16", "classroom_n8_thr02", dict(sampling="fp16"), "fp16 and fp32"),
               ("sampling_fp32", "classroom_n8_thr02", dict(sampling="fp32"), "fp16 and fp32"),
               ("budget_map", "classroom_n8_thr02", dict(), "budget map"),
               ("shard", "classroom_n8_thr02", dict(shard_world=2, shard_rank=0), "shard_world"),
               ("keep_oracle", "classroom_n8_thr02", dict(keep_oracle=True), "fused selection"),
               ("wave_select", "classroom_n8_thr02", dict(wave_select=True), "fused selection")]


@pytest.mark.parametrize("name,case,kw,word", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_unsupported_contexts_are_refused_with_nothing_written(tmp_path_factory, name, case, kw, word):
    z, sc, d = _model(tmp_path_factory, case)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 16), **kw) as r:
        n = r.info.rays_local
        r.set_camera(z["pose"], z["rot"])
        if name == "budget_map":
            r.set_budget_map(np.full(n, 4, np.uint8), None)
        b = Images(r, n)
        d_mask = R.DeviceArray(r, (n,), np.uint8).upload(np.zeros(n, np.uint8))
        try:
            b.install_aux()
            rc, m, _ = masked(r, b, d_mask, 1)
            msg = r.lib.adanerf_last_error(r.handle).decode()
            assert rc == EUNSUPPORTED and m == -7 and "adanerf_render_masked" in msg and word in msg, msg
            assert _untouched(b)
            if name == "budget_map":      # and without the map the same context renders the mask
                r.set_budget_map(None, None)
                rc, m, _ = masked(r, b, d_mask, 1)
                assert rc == 0 and m == n
        finally:
            r.set_aux_outputs(None, None)
            r.set_disp_output(None)
            d_mask.free()
            b.free()


@pytest.mark.parametrize("motion", ["lateral", "yaw20"])
@pytest.mark.parametrize("rerender,selects", [("holes", (0,)), ("unsourced", (0, 2))])
def test_reproject_rerenders_its_holes(model, rerender, selects, motion):
    """NeuralRenderer.reproject_rerender on the reprojection suite's wall + box poses: the plain reprojection with the selected
    pixels replaced by the full render at the destination pose; the frame kept for warping survives"""
    z, sc, d = model
    w, h = 48, 32
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS[motion])
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        r.enable_reprojection()
        r.set_camera(dst[0], dst[1])
        _, fresh, _ = r.render_numpy()
        r.set_camera(src[0], src[1])
        r.render_numpy()
        plain, mask, holes = r.reproject(dst[0], dst[1])
        kept = [a.numpy() for a in (r._rp_depth, r._rp_acc, r._o_rgba)]
        got, mask2, holes2, rerendered = r.reproject_rerender(dst[0], dst[1], rerender)
        sel = np.isin(mask, selects)
        print("%s %s: holes %d, rerendered %d of %d" % (motion, rerender, holes, rerendered, w * h))
        assert holes2 == holes and np.array_equal(mask2, mask) and rerendered == int(sel.sum())
        assert holes > 0 or motion != "yaw20"      # a 20 degree turn uncovers a band of columns no fill reaches
        assert np.array_equal(got, np.where(sel[:, None], fresh, plain))
        for a, b in zip(kept, (r._rp_depth, r._rp_acc, r._o_rgba)):
            assert np.array_equal(bits(a), bits(b.numpy()))
        again, _, _ = r.reproject(dst[0], dst[1])      # the source frame still warps as before
        assert np.array_equal(again, plain)
        with pytest.raises(R.AdaNeRFError):
            r.reproject_rerender(dst[0], dst[1], "everything")


def test_cli_rerender(model, tmp_path):
    """adanerf --reproject 3 --rerender holes|unsourced over a script that turns the camera: every warped frame reports its holes and what was
    rendered into it; with the camera at rest nothing is a hole and the frame is the one --reproject 3 alone shows"""
    import os
    import re
    import subprocess
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    turn, still = tmp_path / "turn.txt", tmp_path / "still.txt"
    turn.write_text("b+ 10 10\nm 40 10\nm 70 14\n")
    still.write_text("# still\n" * 3)
    base = [exe, d, "-s", "64", "48", "-w", "--log-camera", "--reproject", "3"]
    images = {}
    try:
        for script in (turn, still):
            for mode in (None, "holes", "unsourced"):
                out = subprocess.run(base + ["--script", str(script)] + (["--rerender", mode] if mode else []), capture_output=True, text=True, timeout=120)
                assert out.returncode == 0, out.stdout + out.stderr
                images[(script.name, mode)] = open(os.path.join(d, "out.bmp"), "rb").read()
                lines = [re.fullmatch(r"warped (\d+) holes (\d+) rerendered (\d+)", l) for l in out.stdout.splitlines()]
                lines = [tuple(int(v) for v in m.groups()) for m in lines if m]
                print(script.name, mode, lines)
                if mode is None:
                    assert lines == []
                    continue
                assert [l[0] for l in lines] == [1, 2]
                for _, holes, rerendered in lines:
                    assert rerendered == holes if mode == "holes" else rerendered >= holes
                    assert holes == 0 if script is still else True
                if script is turn:
                    assert lines[-1][2] > 0 and images[(script.name, mode)] != images[(script.name, None)]
        for mode in ("holes", "unsourced"):      # at rest every pixel is its own source: nothing to render, the same frame
            assert images[("still.txt", mode)] == images[("still.txt", None)]
    finally:
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))


def test_evaluator_rerender(tmp_path):
    """evaluate(..., reproject_stride=2, rerender=...) on a synthetic 12 x 10 dataset of three poses: every key of the run without the option
    keeps its value, the warped pose gains the score of NeuralRenderer.reproject_rerender's frame"""
    import json
    from adanerf_amd.evaluate import evaluate, psnr_from_mse
    from adanerf_amd.png import read_png, write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h = 12, 10
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    centre = np.array(sc.view_cell_center, np.float32)
    poses = [(centre, O.camera_rotation(100.0, 0.0)), (centre + np.float32([0.05, 0.02, 0.0]), O.camera_rotation(115.0, 0.0)),
             (centre + np.float32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    plain, precs = evaluate(md, str(ds), "test", str(tmp_path / "plain"), precision="bf16", quiet=True, reproject_stride=2)
    for mode in ("holes", "unsourced"):
        summary, recs = evaluate(md, str(ds), "test", str(tmp_path / mode), precision="bf16", quiet=True, reproject_stride=2, rerender=mode)
        assert sorted(summary) == sorted(list(plain) + ["mean_psnr_warped_rerendered", "mean_rerendered_fraction"])
        assert all(summary[k] == plain[k] for k in plain if k != "mean_ms")
        for a, b in zip(recs, precs):
            assert all(a[k] == b[k] for k in b if k != "ms")
        assert [sorted(set(a) - set(b)) for a, b in zip(recs, precs)] == [[], ["mse_rerendered", "psnr_rerendered", "rerendered_fraction"], []]
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
            r.enable_reprojection()
            r.set_camera(*poses[0])
            r.render_numpy()
            want, mask, holes, rerendered = r.reproject_rerender(poses[1][0], poses[1][1], mode)
        assert np.array_equal(read_png(str(tmp_path / mode / "00001_rerendered.png")), want[:, :3].reshape(h, w, 3))
        assert np.array_equal(read_png(str(tmp_path / mode / "00001.png")), read_png(str(tmp_path / "plain" / "00001.png")))
        ref = gts[1].astype(np.float32).reshape(-1, 3) / 255.0
        mse = float(np.mean(((want[:, :3].astype(np.float32) / 255.0).astype(np.float64) - ref) ** 2))
        print("%s: holes %d, rerendered %d of %d, mse %.6f" % (mode, holes, rerendered, w * h, mse))
        assert recs[1]["mse_rerendered"] == mse and recs[1]["psnr_rerendered"] == psnr_from_mse(mse)
        assert recs[1]["rerendered_fraction"] == rerendered / float(w * h) and rerendered == int(np.isin(mask, (0,) if mode == "holes" else (0, 2)).sum())
        assert summary["mean_psnr_warped_rerendered"] == recs[1]["psnr_rerendered"] and summary["mean_rerendered_fraction"] == recs[1]["rerendered_fraction"]
