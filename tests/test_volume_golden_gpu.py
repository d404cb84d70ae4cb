"""The HIP path (through the C-ABI: integration.CubeHandler) against the REFERENCE's own CubeHandler: the cases of
tests/golden/volume_ops_reference.npz (see tests/volume_golden_common.py and tests/test_volume_golden_cpu.py), compared with the fixture alone,
bit for bit after the NaN rule.  Fusion runs through IntegrateImage with PrepareCubes' list checked against the reference's cube_id_list, and
once more through IntegrateCubes over the stored lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import volume_golden_common as V
from onepiece_amd import integration as I


class HipVolume:
    def __init__(self, params, handle=None):
        self.params = params
        if handle is not None:
            self.v = handle
            return
        cam = I.PinholeCamera()
        cam.fx, cam.fy, cam.cx, cam.cy = (float(x) for x in params[:4])
        cam.width, cam.height, cam.depth_scale = int(params[4]), int(params[5]), float(params[6])
        self.v = I.CubeHandler(cam, max_blocks=1 << 12)   # small pool: the larger cases grow it
        self.v.SetVoxelResolution(float(params[7]))
        self.v.SetTruncation(float(params[8]))
        self.v.SetFarPlane(float(params[9]))
        self.v.SetNearPlane(float(params[10]))

    def prepare(self, depth, pose):
        return self.v.PrepareCubes(depth, pose)

    def integrate(self, depth, rgb, pose):
        self.v.IntegrateImage(depth, rgb, pose)

    def integrate_cubes(self, depth, rgb, pose, ids):
        self.v.IntegrateCubes(depth, rgb, pose, ids)
        return True

    def export(self):
        return self.v.GetCubeMap()

    def load(self, keys, vox):
        self.v.SetCubeMap(keys, vox)

    def transform(self, T, nearest):
        return HipVolume(self.params, self.v.TransformNearest(T) if nearest else self.v.Transform(T))

    def resolution(self):
        return self.v.GetVoxelResolution()

    def merge(self, other, T=None):
        before = self.v.GetCubeMap()
        self.v.Merge(other.v, T)
        return other.resolution() != self.resolution() and all(np.array_equal(V.canonical_bits(a) if a.dtype == np.float32 else a,
                                                                              V.canonical_bits(b) if b.dtype == np.float32 else b)
                                                               for a, b in zip(before, self.v.GetCubeMap()))

    def point_cloud(self):
        return self.v.GetPointCloud()

    def mesh(self, tri, pairs, only_block=None):
        return self.v.ExtractTriangleMesh(tri, pairs) if only_block is None else self.v.GenerateMeshByCube(only_block, tri, pairs)

    def count(self):
        return self.v.BlockCount()

    def add_cube(self, key):
        self.v.AddCube(key)

    def write(self, path):
        self.v.WriteToFile(path)

    def read(self, path, legacy=False):
        self.v.ReadFromFileFloat(path) if legacy else self.v.ReadFromFile(path)


def make(params):
    return HipVolume(params)


VOLUMES = ("volume/hand", "volume/fused")


@pytest.mark.parametrize("case", V.case_names("fusion"))
def test_fusion(case):
    V.check_fusion(make, case)


@pytest.mark.parametrize("nearest", [False, True], ids=["trilinear", "nearest"])
@pytest.mark.parametrize("k", range(11), ids=V.TRANSFORM_NAMES)
@pytest.mark.parametrize("case", VOLUMES)
def test_transform(case, k, nearest):
    V.check_transform(make, case, k, nearest)


@pytest.mark.parametrize("case", V.case_names("merge"))
def test_merge(case):
    V.check_merge(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_point_cloud(case):
    V.check_point_cloud(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_mesh(case):
    V.check_mesh(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_add_cube(case):
    V.check_add_cube(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_map_file(case, tmp_path):
    V.check_map_file(make, case, tmp_path)


def test_legacy_float_map(tmp_path):
    V.check_legacy(make, tmp_path)
