// main.cpp of the golden generator (tests/tools/gen_align_color_golden.py): calls the REFERENCE's tool::AlignColorToDepth -- its Tool/IO.cpp,
// Tool/ImageProcessing.cpp, Tool/CppExtension.cpp and Geometry/Geometry.cpp compiled where they lie against the stand-in under opencv2/ -- on
// one image pair per directory: DIR/params.txt, color.u8, depth.f32 | depth.u16 in, DIR/aligned.u8 out (the layout of ScannetIntegration --align).
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "Tool/IO.h"

namespace cv { // never reached by AlignColorToDepth
void pyrDown(const Mat&, Mat&, const Size&) { std::abort(); }
void cvtColor(const Mat&, Mat&, int) { std::abort(); }
void Sobel(const Mat&, Mat&, int, int, int) { std::abort(); }
void GaussianBlur(const Mat&, Mat&, const Size&, double) { std::abort(); }
void bilateralFilter(const Mat&, Mat&, int, double, double) { std::abort(); }
} // namespace cv

using namespace one_piece;

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const std::string dir = argv[a];
        std::ifstream ps((dir + "/params.txt").c_str());
        double c[6], d[7], m[16];
        int rows = 0, cols = 0, u16 = 0;
        for (double& x : c) ps >> x;
        for (double& x : d) ps >> x;
        ps >> rows >> cols >> u16;
        for (double& x : m) ps >> x;
        if (!ps) { std::cerr << "cannot read " << dir << "/params.txt" << std::endl; return 1; }
        camera::PinholeCamera color_camera, depth_camera;
        color_camera.SetPara((float)c[0], (float)c[1], (float)c[2], (float)c[3], (int)c[4], (int)c[5]);
        depth_camera.SetPara((float)d[0], (float)d[1], (float)d[2], (float)d[3], (int)d[4], (int)d[5], (float)d[6]);
        geometry::TransformationMatrix M;
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) M(r, k) = (float)m[4 * r + k];
        cv::Mat color(rows, cols, CV_8UC3), depth((int)d[5], (int)d[4], u16 ? CV_16UC1 : CV_32FC1);
        std::ifstream ic((dir + "/color.u8").c_str(), std::ios::binary), id((dir + (u16 ? "/depth.u16" : "/depth.f32")).c_str(), std::ios::binary);
        ic.read((char*)color.data, (std::streamsize)((size_t)rows * cols * 3));
        id.read((char*)depth.data, (std::streamsize)((size_t)depth.rows * depth.cols * (u16 ? 2 : 4)));
        if (!ic || !id) { std::cerr << "cannot read the images in " << dir << std::endl; return 1; }
        const cv::Mat aligned = tool::AlignColorToDepth(color, depth, color_camera, depth_camera, M);
        std::ofstream os((dir + "/aligned.u8").c_str(), std::ios::binary);
        os.write((const char*)aligned.data, (std::streamsize)((size_t)aligned.rows * aligned.cols * 3));
        if (!os) return 1;
    }
    return 0;
}
