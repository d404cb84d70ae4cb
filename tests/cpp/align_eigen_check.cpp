// align_eigen_check.cpp -- the two Eigen expressions tool::AlignColorToDepth's definition restates, evaluated BY EIGEN (built by
// tests/test_align_color_cpu.py against the real Eigen headers, with the reference's -msse4.2): for every depth pixel with z > 0,
//   p = (T * Vector4(x, y, z, 1)).head<3>() / w        and        uv = (K * (p / p[2])).head<2>()
// so that the evaluation order the restatement claims (sums left to right, three divisions by w, three by p[2], fx * a + cx * c) is pinned by the
// library whose order it is.  Reads DIR/params.txt and the depth image like ScannetIntegration --align; writes DIR/eigen_uv.f32 (h x w x 2).
#include <Eigen/Core>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream ps((dir + "/params.txt").c_str());
    double c[6], d[7], m[16];
    int rows, cols, u16;
    for (double& x : c) ps >> x;
    for (double& x : d) ps >> x;
    ps >> rows >> cols >> u16;
    for (double& x : m) ps >> x;
    if (!ps) return 3;
    const int w = (int)d[4], h = (int)d[5];
    std::vector<float> z((size_t)w * h);
    {
        std::ifstream is((dir + (u16 ? "/depth.u16" : "/depth.f32")).c_str(), std::ios::binary);
        if (u16) {
            std::vector<unsigned short> raw(z.size());
            is.read((char*)raw.data(), (std::streamsize)(raw.size() * 2));
            for (size_t i = 0; i < z.size(); ++i) z[i] = (float)raw[i] / (float)d[6];
        } else {
            is.read((char*)z.data(), (std::streamsize)(z.size() * 4));
        }
        if (!is) return 4;
    }
    Eigen::Matrix4f T;
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) T(r, k) = (float)m[4 * r + k];
    Eigen::Matrix3f K = Eigen::Matrix3f::Zero();
    K(0, 0) = (float)c[0]; K(1, 1) = (float)c[1]; K(0, 2) = (float)c[2]; K(1, 2) = (float)c[3]; K(2, 2) = 1;
    const float fx = (float)d[0], fy = (float)d[1], cx = (float)d[2], cy = (float)d[3];
    std::vector<float> out((size_t)w * h * 2, 0.0f);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const float zz = z[(size_t)i * w + j];
            if (!(zz > 0)) continue;
            const float x = (j - cx) * zz / fx, y = (i - cy) * zz / fy;
            const Eigen::Vector3f point(x, y, zz);
            const Eigen::Vector4f np = T * Eigen::Vector4f(point(0), point(1), point(2), 1.0);
            const Eigen::Vector3f p = np.head<3>() / np(3);
            const Eigen::Vector2f uv = (K * (p / p[2])).head<2>();
            out[((size_t)i * w + j) * 2] = uv(0);
            out[((size_t)i * w + j) * 2 + 1] = uv(1);
        }
    std::ofstream os((dir + "/eigen_uv.f32").c_str(), std::ios::binary);
    os.write((const char*)out.data(), (std::streamsize)(out.size() * 4));
    return os ? 0 : 5;
}
