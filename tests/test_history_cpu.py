"""CPU-only checks of the Python host's history (renderer._History) and of the alpha / depth_tol validator its three users share
(enable_temporal, enable_temporal_upsample, enable_foveated_temporal).  No device: the owner is a stand-in whose arrays record that
they were made and freed.  What the stages compute with these inputs: tests/test_gpu_temporal.py, test_gpu_upsample.py,
test_gpu_sparse_temporal.py."""
import inspect

import numpy as np
import pytest

from adanerf_amd import renderer as R

F32 = np.float32
EXTRAS = [("mask", 1, np.uint8), ("rgba", 4, np.uint8), ("dmask", 1, np.uint8)]      # the foveated stage's: the most any stage names


class FakeArray:
    def __init__(self, log, shape, dtype):
        self.log, self.shape, self.dtype, self.frees = log, tuple(shape), np.dtype(dtype), 0
        log.append(("make", self))

    def free(self):
        self.frees += 1
        self.log.append(("free", self))


class FakeOwner:
    """what _History asks of the renderer: empty(), the list of what it made, the frame present() would show"""

    def __init__(self):
        self.log, self._own, self._last_frame = [], [], None

    def empty(self, shape, dtype):
        a = FakeArray(self.log, shape, dtype)
        self._own.append(a)
        return a

    def made(self):
        return [a for what, a in self.log if what == "make"]


def pose(x=0.25):
    return np.array([x, -1.5, 3.0], F32), np.array([1, 0, 0, 0, 0.6, -0.8, 0, 0.8, 0.6], F32)


@pytest.fixture
def history():
    h = R._History(FakeOwner(), EXTRAS)
    h.ensure(12)
    return h


def test_ensure_makes_two_sets_and_the_extras_at_the_pixel_count(history):
    assert [(a.shape, a.dtype) for st in history.sets for a in st] == [((12, 3), F32), ((12,), F32), ((12,), np.uint8)] * 2
    assert (history.mask.shape, history.rgba.shape, history.dmask.shape) == ((12,), (12, 4), (12,))
    assert {history.mask.dtype, history.rgba.dtype, history.dmask.dtype} == {np.dtype(np.uint8)}
    assert len(history.owner.made()) == 9 and history.owner._own == history.owner.made() == history.buffers()
    history.ensure(12)      # the same count again: nothing made, nothing freed
    assert len(history.owner.log) == 9


def test_the_first_frame_has_no_history_and_writes_set_0(history):
    assert history.hist is None
    assert history.inputs(pose()) == (None, None, None, None, None, history.sets[0])


def test_the_second_frame_reads_set_0_writes_set_1_and_sees_the_committed_pose(history):
    first, second = pose(0.25), pose(0.5)
    history.inputs(first)
    history.commit(first)
    assert history.hist[0] == 0 and history.hist[1] is first[0] and history.hist[2] is first[1]
    rgb, depth, count, prev_pos, prev_rot, out = history.inputs(second)
    assert (rgb, depth, count) == history.sets[0] and out is history.sets[1]
    assert prev_pos is first[0] and prev_rot is first[1]
    history.commit(second)
    rgb, depth, count, prev_pos, prev_rot, out = history.inputs(pose(0.75))      # and back: the sets ping-pong
    assert (rgb, depth, count) == history.sets[1] and out is history.sets[0] and prev_pos is second[0]


@pytest.mark.parametrize("which,element", [(0, 0), (0, 2), (1, 0), (1, 4), (1, 8)])
def test_at_rest_the_depth_input_is_none_and_one_ulp_restores_it(history, which, element):
    at = pose()
    history.commit(at)
    same = (at[0].copy(), at[1].copy())      # bit-identical, not the same objects
    rgb, depth, count, _, _, _ = history.inputs(same)
    assert depth is None and rgb is history.sets[0][0] and count is history.sets[0][2]
    moved = (at[0].copy(), at[1].copy())
    moved[which][element] = np.nextafter(moved[which][element], F32(np.inf))
    assert moved[which][element] != at[which][element]
    assert history.inputs(moved)[:3] == history.sets[0]


def test_reset_makes_the_next_frame_a_first_frame_without_freeing(history):
    history.commit(pose())
    history.reset()
    assert history.hist is None and history.inputs(pose())[:5] == (None,) * 5 and history.inputs(pose())[5] is history.sets[0]
    assert all(a.frees == 0 for a in history.owner.made()) and len(history.owner._own) == 9


@pytest.mark.parametrize("shown", ["rgba", "set", "other", None])
def test_a_new_pixel_count_frees_the_old_buffers_once_and_leaves_no_history(history, shown):
    owner = history.owner
    other = owner.empty((12, 4), np.uint8)      # a buffer of the renderer's that is not the history's
    old = history.buffers()
    frame = {"rgba": history.rgba, "set": history.sets[1][0], "other": other, None: None}[shown]
    owner._last_frame = None if frame is None else (frame, 4, 3)
    history.commit(pose())
    history.ensure(20)
    assert [a.frees for a in old] == [1] * 9 and other.frees == 0
    new = history.buffers()
    assert len(new) == 9 and not set(map(id, new)) & set(map(id, old)) and all(a.frees == 0 and a.shape[0] == 20 for a in new)
    assert owner._own == [other] + new
    assert history.hist is None and history.n == 20
    if shown in ("rgba", "set"):      # present() would have read a freed buffer
        assert owner._last_frame is None
    elif shown == "other":
        assert owner._last_frame == (other, 4, 3)
    else:
        assert owner._last_frame is None


@pytest.mark.parametrize("who", ["enable_temporal", "enable_temporal_upsample", "enable_foveated_temporal"])
def test_the_shared_validator_keeps_the_messages_of_the_three_enable_functions(who):
    assert '_check_blend("%s", alpha, depth_tol)' % who in inspect.getsource(getattr(R.NeuralRenderer, who))      # under its own name
    assert R._check_blend(who, 1, 0) == (1.0, 0.0) and R._check_blend(who, 0.1, 0.02) == (0.1, 0.02)
    assert all(isinstance(v, float) for v in R._check_blend(who, np.float32(0.5), 1))
    for alpha in (0, 0.0, -0.1, 1.0000001, 2, float("nan")):
        with pytest.raises(ValueError) as e:
            R._check_blend(who, alpha, 0.02)
        assert str(e.value) == "%s: alpha must lie in (0, 1], got %r" % (who, alpha)
    for tol in (-1e-9, -1, float("nan")):
        with pytest.raises(ValueError) as e:
            R._check_blend(who, 0.1, tol)
        assert str(e.value) == "%s: depth_tol must be >= 0, got %r" % (who, tol)
    with pytest.raises(ValueError, match="alpha"):      # alpha is looked at first, as before
        R._check_blend(who, 0, -1)
