"""Regenerates tests/golden/align_color_reference.npz: the inputs of tests/align_color_common.py and the aligned images the REFERENCE's own
tool::AlignColorToDepth gives for them.  Build container only: the reference's Tool/IO.cpp, Tool/ImageProcessing.cpp, Tool/CppExtension.cpp and
Geometry/Geometry.cpp (and the jsoncpp IO.cpp links to) are compiled where they lie, against the cv::Mat stand-in of
tests/tools/align_color_golden/opencv2 and the vendored Eigen / Sophus, with the reference's -msse4.2, into oracle/_ref/align_color/.  Only data
is written to the repository.

Left out: depth_height_above_color_rows -- there the reference reads past its colour image (undefined; the one deviation of the definition).

    python tests/tools/gen_align_color_golden.py"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_color_common as A  # noqa: E402

REF = "/root/reference"
LEFT_OUT = ("depth_height_above_color_rows",)


def main():
    here = os.path.join(ROOT, "tests", "tools", "align_color_golden")
    out = os.path.join(ROOT, "oracle", "_ref", "align_color")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "gen_align_color_golden")
    src = [os.path.join(REF, "src", f) for f in ("Tool/IO.cpp", "Tool/ImageProcessing.cpp", "Tool/CppExtension.cpp", "Geometry/Geometry.cpp")]
    src += sorted(glob.glob(os.path.join(REF, "3rdparty", "jsoncpp", "src", "lib_json", "*.cpp")))
    inc = [here, os.path.join(REF, "src"), os.path.join(REF, "src", "Tool"), os.path.join(REF, "3rdparty", "Eigen"), os.path.join(REF, "3rdparty", "Sophus"),
           os.path.join(REF, "3rdparty", "jsoncpp", "include")]
    subprocess.check_call(["g++", "-std=c++11", "-O3", "-msse4.2", "-w"] + ["-I" + i for i in inc] + [os.path.join(here, "main.cpp")] + src + ["-o", exe])
    cases = {n: c for n, c in A.cases().items() if n not in LEFT_OUT}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in cases.items():
            d = os.path.join(tmp, name)
            os.makedirs(d)
            A.write_case(d, case)
        subprocess.check_call([exe] + [os.path.join(tmp, n) for n in cases])
        for name, case in cases.items():
            h, w = case["depth_cam"][5], case["depth_cam"][4]
            arrays[name + "/aligned"] = np.fromfile(os.path.join(tmp, name, "aligned.u8"), np.uint8).reshape(h, w, 3)
            arrays[name + "/color"] = case["color"]
            arrays[name + "/depth"] = case["depth"]
            arrays[name + "/color_cam"] = np.array(case["color_cam"], np.float64)
            arrays[name + "/depth_cam"] = np.array(case["depth_cam"], np.float64)
            arrays[name + "/color_to_depth"] = A.IDENTITY if case["color_to_depth"] is None else case["color_to_depth"]
    path = os.path.join(ROOT, "tests", "golden", "align_color_reference.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d cases, %d bytes)" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
