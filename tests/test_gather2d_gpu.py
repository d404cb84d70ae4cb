"""k_integrate's structured gather (csrc/volume_core.hpp gather2d, through op_debug_gather2d): a buffer descriptor with stride = one image row
and num_records = the rows, read with idxen + offen (vindex = v, voffset = u * 8).

The rule this pins for gfx950 (untyped buffer_load, idxen, stride != 0, swizzling off): the INDEX is compared, unsigned, with num_records and a
row outside [0, height) returns zeros; the OFFSET is not compared with the stride, so gather2d keeps the column test (one compare, one select:
a pixel outside on u reads row -1).  With it the gather returns the pixel's record iff 0 <= u < W and 0 <= v < H, else {0, 0} -- for columns
that would land in the next row under a byte-range rule (2W - 1), for both signs, and at the ends of what project_pixel_uv can return (+-2^23).
test_the_descriptor_alone_checks_the_row_and_not_the_column reads through the descriptor with no column test, on addresses that stay inside
the stack under any rule, and states both halves of the rule as the hardware shows them.

Shapes: 5 x 3, 37 x 29, 64 x 1 (one row) and 2047 x 2 (the widest stride the descriptor's 14-bit field holds); frames 0 and 3 of a stack of
four, so that the base is not the allocation's and the neighbouring frames hold non-zero records a wrong address would return."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import _lib as L

SHAPES = [(5, 3), (37, 29), (64, 1), (2047, 2)]
N_FRAMES = 4


def _vp(a):
    return a.ctypes.data


def _stack(w, h):
    """n_frames x h x w records {depth bits, rgba}: distinct, non-zero in both words."""
    n = N_FRAMES * h * w
    img = np.empty((N_FRAMES, h, w, 2), np.uint32)
    img[..., 0] = (np.arange(n, dtype=np.uint32) + 1).reshape(N_FRAMES, h, w)
    img[..., 1] = (np.arange(n, dtype=np.uint32) + 1).reshape(N_FRAMES, h, w) * np.uint32(2654435761) | np.uint32(1)
    return img


def _gather(img, frame, uv, column_test=1):
    lib = L.load()
    _f, h, w, _two = img.shape
    uv = np.ascontiguousarray(uv, np.int32)
    out = np.full((len(uv), 2), 0xEEEEEEEE, np.uint32)
    L.check(lib.op_debug_gather2d(_vp(img), w, h, N_FRAMES, frame, column_test, _vp(uv), len(uv), _vp(out)))
    return out


@pytest.mark.parametrize("frame", [0, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_record_inside_the_image_zeros_outside(shape, frame):
    w, h = shape
    img = _stack(w, h)
    us = [-2 ** 23, -w - 1, -1, 0, w - 1, w, w + 1, 2 * w - 1, 2 ** 23 - 1]
    vs = [-2 ** 23, -1, 0, h - 1, h, h + 1, 2 ** 23 - 1]
    uv = np.array([(u, v) for v in vs for u in us], np.int32)
    got = _gather(img, frame, uv)
    want = np.zeros_like(got)
    inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    assert inside.sum() == 4                                # u in {0, W - 1} x v in {0, H - 1} (the same row twice when H = 1)
    want[inside] = img[frame, uv[inside, 1], uv[inside, 0]]
    bad = np.nonzero((got != want).any(axis=1))[0]
    for i in bad[:10]:
        print("u %d v %d: got %s, expected %s" % (uv[i, 0], uv[i, 1], got[i], want[i]))
    assert len(bad) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_pixel_of_a_frame_comes_back(shape):
    w, h = shape
    img = _stack(w, h)
    v, u = np.mgrid[0:h, 0:w]
    uv = np.stack([u.ravel(), v.ravel()], axis=1).astype(np.int32)
    assert np.array_equal(_gather(img, 2, uv).reshape(h, w, 2), img[2])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_descriptor_alone_checks_the_row_and_not_the_column(shape):
    """vindex = v, voffset = u * 8 with no column test, on frame 1 of the stack and only where base + v * stride + u * 8 stays inside the
    stack whatever is checked: a row outside [0, H) returns zeros (H, H + 1 and -1, which is frame 0's last row by address); a column W ..
    2W - 1 of a row inside returns the record base + v * stride + u * 8 addresses, in the next row or the next frame."""
    w, h = shape
    img = _stack(w, h)
    flat = img.reshape(-1, 2)
    us = [0, w - 1, w, w + 1, 2 * w - 1]
    uv = np.array([(u, v) for v in (-1, 0, h - 1, h, h + 1) for u in us if 0 <= v < h or u < w], np.int32)
    got = _gather(img, 1, uv, column_test=0)
    row_ok = (uv[:, 1] >= 0) & (uv[:, 1] < h)
    want = np.zeros_like(got)
    want[row_ok] = flat[(h + uv[row_ok, 1]) * w + uv[row_ok, 0]]
    assert (uv[row_ok, 0] >= w).sum() == 6 and (want[row_ok] != 0).all()
    bad = np.nonzero((got != want).any(axis=1))[0]
    for i in bad[:10]:
        print("u %d v %d: got %s, expected %s" % (uv[i, 0], uv[i, 1], got[i], want[i]))
    assert len(bad) == 0


def test_arguments_outside_the_contract_are_refused():
    lib = L.load()
    img = _stack(5, 3)
    out = np.zeros((1, 2), np.uint32)
    for uv in ([2 ** 23, 0], [0, -2 ** 23 - 1]):
        a = np.array([uv], np.int32)
        assert lib.op_debug_gather2d(_vp(img), 5, 3, N_FRAMES, 0, 1, _vp(a), 1, _vp(out)) != 0
    a = np.zeros((1, 2), np.int32)
    assert lib.op_debug_gather2d(_vp(img), 2048, 1, 1, 0, 1, _vp(a), 1, _vp(out)) != 0   # a row the stride field cannot hold
    assert lib.op_debug_gather2d(_vp(img), 5, 3, N_FRAMES, N_FRAMES, 1, _vp(a), 1, _vp(out)) != 0
    for uv in ([-1, 0], [0, 3 * N_FRAMES]):                                            # the descriptor alone: an address outside the stack
        a = np.array([uv], np.int32)
        assert lib.op_debug_gather2d(_vp(img), 5, 3, N_FRAMES, 0, 0, _vp(a), 1, _vp(out)) != 0
