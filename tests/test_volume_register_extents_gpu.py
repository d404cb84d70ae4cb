"""How far the one-pass entries of op_volume_register_* write, and that the narrow ones are prefixes of the wide one.

Every one-pass entry runs the same host path and copies out what its own signature promises: op_volume_register_system 28 sums, 4 counts and rows of 8,
op_volume_register_color_system 30, 5 and rows of 16, op_volume_register_robust_system (the reference here, with all-zero options) 31, 7 and rows of
16, op_volume_register_batch_system 31 and 7 per cloud.  The caller's buffers carry guard values behind those extents; the values in front of them
are compared as bit patterns.

Scene: the hand-made blocks of the register tests.  Clouds of 0, 1, 255, 256, 257 points (nothing, one lane, one workgroup's edge either side) and of
1024 * 256 + 1, the smallest that passes the grid cap; each with OP_MEM_HOST and OP_MEM_DEVICE, with and without rows."""
import ctypes as C

import numpy as np
import pytest

import deintegrate_common as D
import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (0, 1, 255, 256, 257, 1024 * 256 + 1)
BEFORE, AFTER = 300, 65                                               # the clouds either side of the one under test in the batch call
GATE, LIMIT = 0.25, 0.05
GUARD, PAD = 7.0, 4
_cache = {}


def _scene():
    """-> dict(hv, q, y): the hand-made blocks and one hand cloud every cloud of the tests is cut from, with intensities"""
    if "scene" not in _cache:
        hcam = I.PinholeCamera()
        hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = D.CAM_37
        hv = I.CubeHandler(hcam, device=0, max_blocks=1 << 13)
        hv.SetVoxelResolution(R.HAND_RES)
        hv.SetTruncation(B.TRUNC)
        hv.AddCubes(R.HAND_KEYS, B.steep_blocks(color=True))
        total = BEFORE + max(SIZES) + AFTER
        q = R.hand_cloud(n=total - len(R.HAND_POINTS))
        idx = np.arange(total)
        with np.errstate(all="ignore"):
            c = F32(0.5) + q[:, 0]
            y = K.intensity(np.stack([c, c, c], axis=1))
        y[idx % 2 == 0] += F32(0.03125)
        y[idx % 5 == 0] += F32(0.0625)                                # gated by LIMIT
        y[idx % 16 == 1] = np.nan
        _cache["scene"] = dict(hv=hv, q=np.ascontiguousarray(q), y=np.ascontiguousarray(y, F32))
    return _cache["scene"]


def _pose(c):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = [(c % 3) / 128, 0.0, -(c % 4) / 128]
    return T.reshape(16)


_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_up = lambda a: a.ctypes.data_as(L._u64p)
_fp = lambda a: a.ctypes.data_as(L._fp)
_vp = lambda a: C.c_void_p(a.ctypes.data)
_bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)
_bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _want(n, cs):
    """op_volume_register_robust_system with all-zero options on the cloud of n points (host memory, with rows), computed once -> (sums [31], counts [7], rows [n,16])"""
    if (n, cs) not in _cache:
        s = _scene()
        q, y = s["q"][BEFORE:BEFORE + n], s["y"][BEFORE:BEFORE + n]
        sums, counts, rows = np.zeros(31), np.zeros(7, np.uint64), np.zeros((n, 16), F32)
        opt = L.RegisterOptions(L.OP_REGISTER_LIN_NORMAL, 0.0, 0.0)
        L.check(L.load().op_volume_register_robust_system(s["hv"]._h, _vp(q), _vp(y), n, L.OP_MEM_HOST, _fp(_pose(1)), GATE, cs, LIMIT, C.byref(opt), _dp(sums), _up(counts),
                                                          _vp(rows)))
        _cache[(n, cs)] = (sums, counts, rows)
    return _cache[(n, cs)]


class _Buffers:
    """the caller's side of one call: sums and counts with PAD guard values behind their extent, rows with PAD guard rows behind row n, in `mem`"""

    def __init__(self, n, n_sums, n_counts, row_w, mem, with_rows):
        self.n, self.n_sums, self.n_counts, self.row_w, self.mem = n, n_sums, n_counts, row_w, mem
        self.sums = np.full(n_sums + PAD, GUARD)
        self.counts = np.full(n_counts + PAD, int(GUARD), np.uint64)
        self.rows = None
        if with_rows and mem == L.OP_MEM_HOST:
            self.rows = np.full((n + PAD, row_w), GUARD, F32)
            self.rows_ptr = _vp(self.rows)
        elif with_rows:
            import torch
            self.rows = torch.full((n + PAD, row_w), GUARD, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            self.rows_ptr = C.c_void_p(self.rows.data_ptr())
        else:
            self.rows_ptr = None

    def check(self, want, what):
        sums, counts, rows = want
        assert np.array_equal(_bits64(self.sums[:self.n_sums]), _bits64(sums[:self.n_sums])), (what, self.sums, sums)
        assert np.array_equal(self.counts[:self.n_counts], counts[:self.n_counts]), (what, self.counts, counts)
        assert (self.sums[self.n_sums:] == GUARD).all() and (self.counts[self.n_counts:] == int(GUARD)).all(), (what, self.sums, self.counts)
        if self.rows is not None:
            got = self.rows if self.mem == L.OP_MEM_HOST else self.rows.cpu().numpy()
            assert np.array_equal(_bits(got[:self.n]), _bits(rows[:, :self.row_w])), what
            assert (got[self.n:] == F32(GUARD)).all(), what


def _inputs(q, y, mem):
    """-> (xyz pointer, intensity pointer, what keeps them alive)"""
    if mem == L.OP_MEM_HOST:
        return _vp(q), _vp(y), (q, y)
    import torch
    dq, dy = torch.from_numpy(q).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    return C.c_void_p(dq.data_ptr()), C.c_void_p(dy.data_ptr()), (dq, dy)


@pytest.mark.parametrize("with_rows", [False, True], ids=["sums", "rows"])
@pytest.mark.parametrize("mem", [L.OP_MEM_HOST, L.OP_MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_narrow_entries_write_their_prefix_and_nothing_more(n, mem, with_rows):
    s = _scene()
    hv, lib = s["hv"], L.load()
    q, y = s["q"][BEFORE:BEFORE + n], s["y"][BEFORE:BEFORE + n]
    px, py, keep = _inputs(q, y, mem)
    T = _pose(1)
    geo = _want(n, 0.0)
    assert not geo[2][:, 8:].any()                                    # no colour term: the second halves of the rows of 16 are zero
    if n == max(SIZES):                                               # the comparison is not between zeros
        assert min(int(c) for c in geo[1][:4]) > 0 and geo[0][27] > 0 and int(_want(n, 1.0)[1][4]) > 0 and int(geo[1][4]) == 0
    b = _Buffers(n, 28, 4, 8, mem, with_rows)
    L.check(lib.op_volume_register_system(hv._h, px, n, mem, _fp(T), GATE, _dp(b.sums), _up(b.counts), b.rows_ptr))
    b.check(geo, "op_volume_register_system n=%d" % n)
    for cs in (0.0, 1.0):
        b = _Buffers(n, 30, 5, 16, mem, with_rows)
        L.check(lib.op_volume_register_color_system(hv._h, px, py, n, mem, _fp(T), GATE, cs, LIMIT, _dp(b.sums), _up(b.counts), b.rows_ptr))
        b.check(_want(n, cs), "op_volume_register_color_system n=%d color_scale %g" % (n, cs))
    del keep


@pytest.mark.parametrize("mem", [L.OP_MEM_HOST, L.OP_MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_a_batch_row_is_the_single_call_whatever_stands_beside_it(n, mem):
    s = _scene()
    hv, lib = s["hv"], L.load()
    opt = L.RegisterOptions(L.OP_REGISTER_LIN_NORMAL, 0.0, 0.0)
    for cs in (0.0, 1.0):
        want = _want(n, cs)
        for a, starts, c in ((BEFORE, [0, n], 0), (0, [0, BEFORE, BEFORE + n, BEFORE + n + AFTER], 1)):   # alone; between two others
            st = np.array(starts, np.uint64)
            nc = len(st) - 1
            q, y = s["q"][a:a + int(st[-1])], s["y"][a:a + int(st[-1])]
            px, py, keep = _inputs(q, y, mem)
            T = np.stack([_pose(1 if k == c else 2 + k) for k in range(nc)])
            sums, counts = np.full(31 * nc + PAD, GUARD), np.full(7 * nc + PAD, int(GUARD), np.uint64)
            L.check(lib.op_volume_register_batch_system(hv._h, px, None, py, _up(st), nc, mem, _fp(T), GATE, cs, LIMIT, C.byref(opt), _dp(sums), _up(counts)))
            what = "n=%d color_scale %g cloud %d of %d" % (n, cs, c, nc)
            assert np.array_equal(_bits64(sums[31 * c:31 * c + 31]), _bits64(want[0])), (what, sums[31 * c:31 * c + 31], want[0])
            assert np.array_equal(counts[7 * c:7 * c + 7], want[1]), (what, counts[7 * c:7 * c + 7], want[1])
            assert (sums[31 * nc:] == GUARD).all() and (counts[7 * nc:] == int(GUARD)).all(), what
            del keep
