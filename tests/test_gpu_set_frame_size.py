"""adanerf_set_frame_size on the GPU: after a change of the frame size a context must be indistinguishable from a context created with
the same options at that size -- RGBA8, fp32 RGB, depth / acc / disp (set again for the new size), the ray counts, adanerf_info field
by field and the sample total, byte for byte (the library is deterministic: there is no tolerance anywhere in this file).  Sizes: 97 x 61
and 131 x 67 are no multiple of 32, 128 or the 256-sample shading tile; 8 x 8 and 1 x 1 are less than one tile.  Run with
`pytest -m gpu` on an MI355X box."""
import ctypes as C

import numpy as np
import pytest

import adanerf_oracle as O
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = dict(sampling="guarded", guard_eps=1e-2, guard_eps_pair=1.5e-2, guard_cache=False)      # explicit bounds: nothing calibrates

# kind -> (golden fixture, num_samples, threshold, renderer keywords)
KINDS = {
    "split": ("classroom_n8_thr02", 8, 0.2, dict(sampling="split")),
    "fp32": ("classroom_n8_thr02", 8, 0.2, dict(sampling="fp32")),
    "fp16": ("classroom_n8_thr02", 8, 0.2, dict(sampling="fp16")),
    "guarded": ("classroom_n8_thr02", 8, 0.2, GUARD),
    "dense": ("classroom_n8_thr02", 128, 0.0, {}),
    "pdf": ("classroom_pdf_n8", 8, -1.0, {}),
    "coarse_fine": ("classroom_coarse_fine_16_24", 0, -1.0, {}),
    "ndc": ("ndc_synthetic_n8", 0, -1.0, {}),
    "topology": ("syn_w40_w70_skip1", 8, 0.2, {}),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """fixture name -> (fixture arrays, model directory), written here from the seeded scenes and weights of the golden fixtures"""
    out = {}
    for name in sorted({v[0] for v in KINDS.values()}):
        z, meta, sc = load_case(name)
        d = str(tmp_path_factory.mktemp("size_" + name))
        O.write_model_dir(d, sc, case_weights(meta))
        out[name] = (z, d)
    return out


class Ctx:
    """A renderer of one kind with every output attached, and a snapshot of all a frame leaves behind."""

    def __init__(self, models, kind, w, h, **kw):
        name, n, thr, base = KINDS[kind]
        self.z, d = models[name]
        kw = dict(base, **kw)
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=kw.pop("batch_size", -1)), num_samples=n, threshold=thr, **kw)
        self.r.init()
        self.r.set_camera(self.z["pose"], self.z["rot"])
        self.aux = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()

    def attach(self):
        """depth / acc / disp buffers for the rays_local in force, set (again)"""
        nl = self.r.refresh_info().rays_local
        self.aux = [self.r.empty((nl,), np.float32) for _ in range(3)]
        self.r.set_aux_outputs(self.aux[0], self.aux[1])
        self.r.set_disp_output(self.aux[2])

    def frame(self):
        r = self.r
        self.attach()
        for a in self.aux:      # a ray the frame does not write must not pass for equal by accident
            a.upload(np.full(a.shape, -7.0, np.float32))
        rgb, rgba, st = r.render_numpy()
        info = r.refresh_info()
        nl, nb = info.rays_local, info.batch_rays
        last = nl - ((nl - 1) // nb) * nb if nl else 0      # the buffers hold the frame's last batch
        return dict(rgba=rgba, rgb=rgb, depth=self.aux[0].numpy(), acc=self.aux[1].numpy(), disp=self.aux[2].numpy(),
                    counts=r.buffer(R.BUF_RAY_COUNTS, np.int32, (last,)), info=np.frombuffer(bytes(info), np.uint8).copy(),
                    total_samples=np.int64(st.total_samples), refined=np.int64(st.rays_refined))


def same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for name, _ in R.Info._fields_:      # field by field first: a readable failure
        fa, fb = (getattr(R.Info.from_buffer_copy(x["info"].tobytes()), name) for x in (a, b))
        assert bytes(fa) == bytes(fb) if hasattr(fa, "_length_") else fa == fb, "%s: adanerf_info.%s %r != %r" % (what, name, fa, fb)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


_fresh = {}


def fresh(models, kind, w, h, **kw):
    """the frame of a context created at w x h (computed once per module and shared)"""
    key = (kind, w, h, tuple(sorted(kw.items())))
    if key not in _fresh:
        with Ctx(models, kind, w, h, **kw) as c:
            _fresh[key] = c.frame()
    return _fresh[key]


def walk(models, kind, sizes, **kw):
    """create at sizes[0], then every later size on the one context; after each step: the fresh context's frame"""
    w0, h0 = sizes[0]
    with Ctx(models, kind, w0, h0, **kw) as c:
        first = c.frame()
        same(first, fresh(models, kind, w0, h0, **kw), "%s start %dx%d" % (kind, w0, h0))
        for w, h in sizes[1:]:
            info = c.r.set_frame_size(w, h)
            assert (info.width, info.height) == (w, h) and c.r.info is info and (c.r.settings.width, c.r.settings.height) == (w, h)
            got = c.frame()
            same(got, fresh(models, kind, w, h, **kw), "%s after set_frame_size(%d, %d)" % (kind, w, h))
        if sizes[-1] == sizes[0]:
            same(got, first, "%s back at %dx%d" % (kind, w0, h0))


@pytest.mark.parametrize("sizes", [[(97, 61), (64, 48), (97, 61)], [(8, 8), (131, 67)], [(131, 67), (1, 1)]],
                         ids=["ragged-shrink-back", "grow", "to-one-pixel"])
def test_size_chains(models, sizes):
    walk(models, "split", sizes)


def test_a_non_positive_value_keeps_that_side(models):
    with Ctx(models, "split", 97, 61) as c:
        assert c.r.lib.adanerf_set_frame_size(c.r.handle, -1, 48) == 0
        assert (c.r.refresh_info().width, c.r.info.height) == (97, 48)
        same(c.frame(), fresh(models, "split", 97, 48), "(-1, 48)")
        assert c.r.lib.adanerf_set_frame_size(c.r.handle, 64, 0) == 0
        same(c.frame(), fresh(models, "split", 64, 48), "(64, 0)")
        info = c.r.set_frame_size(None, 61)
        assert (info.width, info.height) == (64, 61)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_kind_follows_the_size(models, kind):
    """a shrink, then a growth past the size the context was created with"""
    walk(models, kind, [(97, 61), (64, 48), (131, 67)])


def test_guarded_audit_starts_over(models):
    """Frames do not depend on the audit's phase, and a size change starts it over: after two frames at one size (the audit has moved on)
    the first frame at the next size equals the FIRST frame of a fresh guarded context there, re-evaluated rays included."""
    with Ctx(models, "guarded", 97, 61) as c:
        a0 = c.frame()
        assert 0 < a0["refined"] < 97 * 61
        a1 = c.frame()
        assert a1["rgba"].tobytes() == a0["rgba"].tobytes() and a1["counts"].tobytes() == a0["counts"].tobytes()
        c.r.set_frame_size(64, 48)
        same(c.frame(), fresh(models, "guarded", 64, 48), "guarded 64x48 after two frames at 97x61")
        assert c.r.info.guard_eps == np.float32(1e-2) and c.r.info.guard_calib_source == 1      # the band is the model's: it stays


def test_batch_is_derived_from_the_request(models):
    """-bs 1000 on an 8 x 8 frame runs batches of 64; at 97 x 61 the batch is the 1000 the caller asked for, not the clamped 64."""
    with Ctx(models, "split", 8, 8, batch_size=1000) as c:
        assert c.r.info.batch_rays == 64
        c.frame()
        info = c.r.set_frame_size(97, 61)
        assert info.batch_rays == 1000
        want = fresh(models, "split", 97, 61, batch_size=1000)
        assert R.Info.from_buffer_copy(want["info"].tobytes()).batch_rays == 1000
        same(c.frame(), want, "batch 1000, 8x8 -> 97x61")
        assert want["rgba"].tobytes() == fresh(models, "split", 97, 61)["rgba"].tobytes()      # and batching does not change the frame


def test_three_shards_resized_assemble_to_the_unsharded_frame(models):
    kw = dict(shard_world=3, strip_rows=5)
    ranks = [Ctx(models, "split", 97, 61, shard_rank=k, **kw) for k in range(3)]
    try:
        parts = []
        for k, c in enumerate(ranks):
            c.frame()
            c.r.set_frame_size(64, 48)
            got = c.frame()
            same(got, fresh(models, "split", 64, 48, shard_rank=k, **kw), "rank %d of 3 at 64x48" % k)
            pad = np.zeros((c.r.info.rays_local_max, 4), np.uint8)
            pad[:got["rgba"].shape[0]] = got["rgba"]
            parts.append(pad)
        assert sum(c.r.info.rays_local for c in ranks) == 64 * 48
        r0 = ranks[0].r
        img = r0.empty((64 * 48, 4), np.uint8)
        r0.assemble_strips(r0.to_device(np.concatenate(parts)), img)
        r0.sync()
        assert np.array_equal(img.numpy(), fresh(models, "split", 64, 48)["rgba"])
    finally:
        for c in ranks:
            c.r.close()


def test_a_refused_size_leaves_everything(models):
    """what adanerf_create refuses, with its code and message; then the same info and the same frame"""
    for kind, w, h, text in (("split", 8192, 4096, "width*height must be < 2^25"), ("dense", 8192, 4095, "batch_rays * num_samples exceeds 2^31 - 1")):
        with Ctx(models, kind, 64, 48) as c:
            before = c.frame()
            ptrs = buffer_pointers(c.r)
            assert c.r.lib.adanerf_set_frame_size(c.r.handle, w, h) == EINVAL, (kind, w, h)
            msg = c.r.lib.adanerf_last_error(c.r.handle).decode()
            assert text in msg, msg
            name, n, thr, base = KINDS[kind]
            with pytest.raises(R.AdaNeRFError) as e:
                adanerf_amd.NeuralRenderer(adanerf_amd.Settings(models[name][1], w, h), num_samples=n, threshold=thr, **base).init()
            assert msg in str(e.value) and "(%d)" % EINVAL in str(e.value)
            assert buffer_pointers(c.r) == ptrs
            same(c.frame(), before, "%s after the refused %dx%d" % (kind, w, h))
            with pytest.raises(R.AdaNeRFError):
                c.r.set_frame_size(w, h)
            assert (c.r.settings.width, c.r.settings.height, c.r.info.width, c.r.info.height) == (64, 48, 64, 48)


def buffer_pointers(r):
    out = []
    for which in range(10):
        p, nb = C.c_void_p(), C.c_size_t()
        assert r.lib.adanerf_get_buffer(r.handle, which, C.byref(p), C.byref(nb)) == 0
        out.append((p.value, nb.value))
    return out


@pytest.mark.parametrize("kind", ["split", "guarded", "coarse_fine"])
def test_buffers_move_only_when_they_grow(models, kind):
    with Ctx(models, kind, 97, 61) as c:
        c.frame()
        start = buffer_pointers(c.r)
        c.r.set_frame_size(97, 61)
        assert buffer_pointers(c.r) == start, "same size"
        c.r.set_frame_size(64, 48)
        c.frame()
        assert buffer_pointers(c.r) == start, "shrink"
        c.r.set_frame_size(90, 65)      # 5 850 rays <= the 5 917 held
        c.frame()
        assert buffer_pointers(c.r) == start, "growth within the largest batch held"
        c.r.set_frame_size(97, 61)
        assert buffer_pointers(c.r) == start, "back"
        c.r.set_frame_size(131, 67)
        grown = buffer_pointers(c.r)
        assert all(g[1] >= s[1] for g, s in zip(grown, start)) and any(g[1] > s[1] for g, s in zip(grown, start))
        c.frame()
        c.r.set_frame_size(8, 8)
        c.r.set_frame_size(131, 67)
        c.frame()
        assert buffer_pointers(c.r) == grown, "render allocates nothing; capacities never shrink"


def test_resizes_return_all_device_memory(models):
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def cycle():
        for kind in ("split", "guarded", "pdf", "coarse_fine"):
            with Ctx(models, kind, 40, 30) as c:
                for w, h in ((131, 67), (8, 8), (160, 120), (97, 61)):
                    c.r.set_frame_size(w, h)
                    c.frame()

    cycle()                                   # first use: HIP's own caches (code objects, pools) fill up
    base = free_bytes()
    for _ in range(3):
        cycle()
    assert abs(free_bytes() - base) <= 8 << 20, (base, free_bytes())      # as test_context_lifecycle_returns_all_device_memory


def test_enqueued_frames_keep_their_size(models):
    """render into A at 64 x 48, grow to 131 x 67, render into B, one sync at the end"""
    with Ctx(models, "split", 64, 48) as c:
        r = c.r
        a, b = r.empty((64 * 48, 4), np.uint8), r.empty((131 * 67, 4), np.uint8)
        r.render(a, None)
        r.set_frame_size(131, 67)
        r.render(b, None)
        r.sync()
        assert a.numpy().tobytes() == fresh(models, "split", 64, 48)["rgba"].tobytes()
        assert b.numpy().tobytes() == fresh(models, "split", 131, 67)["rgba"].tobytes()
        assert np.array_equal(r.present(131, 67), b.numpy().reshape(67, 131, 4))      # the camera in force stayed; equal sizes: identity


def test_per_ray_outputs_are_dropped_only_when_rays_local_changes(models):
    with Ctx(models, "split", 97, 61) as c:
        r = c.r
        depth = r.empty((97 * 61,), np.float32)
        canary = np.full((97 * 61,), -7.0, np.float32)
        out = r.empty((97 * 61, 4), np.uint8)
        r.set_aux_outputs(depth.upload(canary), None)
        r.set_frame_size(61, 97)      # another image, the same number of rays: the buffer still fits and stays set
        r.render(out, None)
        r.sync()
        got = depth.numpy()
        assert not np.any(got == -7.0)
        with Ctx(models, "split", 61, 97) as f:
            f.attach()
            f.r.render_numpy()
            assert got.tobytes() == f.aux[0].numpy().tobytes()
        r.set_frame_size(64, 48)      # fewer rays: the outputs are reset to NULL
        depth.upload(canary)
        r.render(out, None)
        r.sync()
        assert np.array_equal(depth.numpy(), canary)
