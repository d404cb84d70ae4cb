// IO.cpp -- tool::ReadImageSequence / ReadImageSequenceWithPose: the reference's sequence directory format; the ScanNet layout's readers;
// tool::AlignColorToDepth.
#include "Tool/IO.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "Bridge.h"

namespace one_piece {
namespace tool {

void ReadImageSequence(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files) {
    std::ifstream in((path + "/associate.txt").c_str());
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string t_rgb, rgb, t_depth, depth;
        fields >> t_rgb >> rgb >> t_depth >> depth; // a short line yields empty names, as the reference's parser does
        rgb_files.push_back(path + "/" + rgb);
        depth_files.push_back(path + "/" + depth);
    }
    std::cout << GREEN << "[ReadImageSequence]::[INFO]::Read " << rgb_files.size() << " images successfully." << RESET << std::endl;
}

void ReadImageSequenceWithPose(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                               std::vector<geometry::TransformationMatrix>& poses) {
    std::ifstream in((path + "/trajectory.txt").c_str());
    if (!in) {
        std::cout << RED << "[ReadImageSequenceWithPose]::[ERROR]::No file named trajectory.txt." << RESET << std::endl;
        return;
    }
    ReadImageSequence(path, rgb_files, depth_files);
    std::string line;
    geometry::TransformationMatrix pose; // a short line keeps the previous line's trailing entries, like the reference's reused matrix
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) fields >> pose(r, c);
        poses.push_back(pose);
    }
    if (poses.size() != rgb_files.size())
        std::cout << YELLOW << "[ReadImageSequenceWithPose]::[WARNING]:: The number of images and poses do not match." << RESET << std::endl;
}

// The reference's loop (IO.cpp:9-58 over Geometry.cpp:29-34,94-96) with its quirks kept; see DESIGN.md section 0.  float32 throughout, every product,
// quotient and sum rounded on its own (x86-64 without FMA code generation: nothing contracts), sums in the order Eigen's fixed-size products take.
static void AlignColorToDepthHost(const cv::Mat& color, const cv::Mat& depth, const op_camera& cc, const op_camera& dc, const float M[16], cv::Mat& aligned) {
    const int u_lim = cc.width < color.cols ? cc.width : color.cols;
    // IO.cpp:33: the vertical bound is the DEPTH camera's height.  Where that exceeds the colour image's rows the reference reads past its image;
    // here such a pixel is rejected.
    const int v_lim = dc.height < color.rows ? dc.height : color.rows;
    const bool u16 = depth.depth() != CV_32F;
    for (int v = 0; v < depth.rows; ++v) { // :41-43: the loop runs over the depth IMAGE, the output has the depth CAMERA's size
        for (int u = 0; u < depth.cols; ++u) {
            const size_t pix = static_cast<size_t>(v) * depth.cols + u;
            const float z = u16 ? static_cast<float>(reinterpret_cast<const unsigned short*>(depth.data)[pix]) / dc.depth_scale : reinterpret_cast<const float*>(depth.data)[pix];
            if (!(z > 0)) continue;                                                        // :46 (a NaN fails it too)
            const float x = (static_cast<float>(u) - dc.cx) * z / dc.fx;                    // Geometry.cpp:94-96
            const float y = (static_cast<float>(v) - dc.cy) * z / dc.fy;
            float q[4];
            for (int r = 0; r < 4; ++r) q[r] = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] * 1.0f;   // Geometry.cpp:31-32
            const float p0 = q[0] / q[3], p1 = q[1] / q[3], p2 = q[2] / q[3];               // :33
            const float a = p0 / p2, b = p1 / p2, c = p2 / p2;                              // IO.cpp:49
            const float uf = cc.fx * a + cc.cx * c;
            const float vf = cc.fy * b + cc.cy * c;
            const double du = static_cast<double>(uf) + 0.5, dv = static_cast<double>(vf) + 0.5;   // :50-51
            // a NaN, or a value whose truncation is no int, is undefined in the cast (x86 gives INT_MIN, which fails the bound): rejected
            if (!(du > -2147483649.0 && du < 2147483648.0 && dv > -2147483649.0 && dv < 2147483648.0)) continue;
            const int cu = static_cast<int>(du), cv_ = static_cast<int>(dv);
            if (cu < 0 || cu >= u_lim || cv_ < 0 || cv_ >= v_lim) continue;                  // :52
            const unsigned char* s = color.data + 3 * (static_cast<size_t>(cv_) * color.cols + cu);
            unsigned char* o = aligned.data + 3 * (static_cast<size_t>(v) * dc.width + u);
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        }
    }
}

cv::Mat AlignColorToDepth(const cv::Mat& color, const cv::Mat& depth, const camera::PinholeCamera& rgb_camera, const camera::PinholeCamera& depth_camera,
                          const geometry::TransformationMatrix& color_to_depth) {
    if (depth.depth() != CV_16U && depth.depth() != CV_32F) {
        std::cout << RED << "[ImageProcessing]::[ERROR]::Unknown depth image type: " << depth.depth() << RESET << std::endl;
        std::exit(1);
    }
    const op_camera &cc = rgb_camera.Pod(), &dc = depth_camera.Pod();
    const int h = dc.height > 0 ? dc.height : 0, w = dc.width > 0 ? dc.width : 0;
    cv::Mat aligned(h, w, CV_8UC3);
    if (aligned.data) std::memset(aligned.data, 0, aligned.total() * 3);
    if (depth.empty() || color.empty() || color.type() != CV_8UC3 || depth.rows > h || depth.cols > w) {
        // (the reference walks the depth IMAGE and writes into an image of the CAMERA's size: a larger depth image writes past it there)
        std::cout << RED << "[ERROR]::[AlignColorToDepth]::the depth image must fit the depth camera's size, the colour image needs three byte channels." << RESET << std::endl;
        return aligned;
    }
    float M[16];
    bridge::RowMajor(color_to_depth, M);
    // the device entry takes a depth image of exactly the camera's size (it is told no other): a smaller one is the host loop's
    if (bridge::DeviceColorAlignment() && depth.rows == h && depth.cols == w) {
        const int rc = op_align_color_to_depth(&cc, &dc, color.data, color.rows, color.cols, depth.data, bridge::DepthFormat(depth), M, OP_MEM_HOST, bridge::Device(),
                                               aligned.data);
        if (rc != OP_ERR_INVALID && rc != OP_ERR_CAPACITY) {
            if (bridge::Failed(rc, "AlignColorToDepth")) std::memset(aligned.data, 0, aligned.total() * 3);
            return aligned;
        }
        std::memset(aligned.data, 0, aligned.total() * 3);
    }
    AlignColorToDepthHost(color, depth, cc, dc, M, aligned);
    return aligned;
}

// "a<delim>b<delim>c" -> the non-empty pieces
static std::vector<std::string> SplitNonEmpty(const std::string& s, const std::string& delim) {
    std::vector<std::string> out;
    size_t start = 0;
    while (start <= s.size()) {
        const size_t at = s.find(delim, start);
        const size_t end = at == std::string::npos ? s.size() : at;
        if (end > start) out.push_back(s.substr(start, end - start));
        if (at == std::string::npos) break;
        start = at + delim.size();
    }
    return out;
}

void ReadImageSequenceFromScannet(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                                  camera::PinholeCamera& rgb_camera, camera::PinholeCamera& depth_camera) {
    std::ifstream in((path + "/_info.txt").c_str());
    int color_width = -1, color_height = -1, depth_width = -1, depth_height = -1, depth_scale = -1;
    size_t frames = 0;
    float kc[4] = {0, 0, 0, 0}, kd[4] = {0, 0, 0, 0}; // fx, cx, fy, cy
    std::string line;
    while (std::getline(in, line)) {
        const std::vector<std::string> kv = SplitNonEmpty(line, " = ");
        const std::string key = kv.size() == 2 ? kv[0] : std::string();
        if (key == "m_versionNumber" || key == "m_sensorName" || key == "m_calibrationColorExtrinsic" || key == "m_calibrationDepthExtrinsic") continue;
        if (key == "m_colorWidth") color_width = std::atoi(kv[1].c_str());
        else if (key == "m_colorHeight") color_height = std::atoi(kv[1].c_str());
        else if (key == "m_depthWidth") depth_width = std::atoi(kv[1].c_str());
        else if (key == "m_depthHeight") depth_height = std::atoi(kv[1].c_str());
        else if (key == "m_depthShift") depth_scale = std::atoi(kv[1].c_str());
        else if (key == "m_frames.size") frames = static_cast<size_t>(std::atoi(kv[1].c_str()));
        else if (key == "m_calibrationColorIntrinsic" || key == "m_calibrationDepthIntrinsic") {
            const std::vector<std::string> t = SplitNonEmpty(kv[1], " ");
            float* k = key == "m_calibrationColorIntrinsic" ? kc : kd;
            if (t.size() > 6) { k[0] = static_cast<float>(std::atof(t[0].c_str())); k[1] = static_cast<float>(std::atof(t[2].c_str())); k[2] = static_cast<float>(std::atof(t[5].c_str())); k[3] = static_cast<float>(std::atof(t[6].c_str())); }
        } else { // a line that does not split in two, or an unknown key: the warning, and the parse ENDS (what was read so far is kept)
            std::cout << YELLOW << "[Warning]::[ReadImageSequenceFromScannet]::Wrong format of _info.txt" << RESET << std::endl;
            break;
        }
    }
    rgb_camera.SetPara(kc[0], kc[2], kc[1], kc[3], color_width, color_height);
    depth_camera.SetPara(kd[0], kd[2], kd[1], kd[3], depth_width, depth_height, static_cast<float>(depth_scale));
    rgb_files.clear();
    depth_files.clear();
    for (size_t i = 0; i != frames; ++i) {
        char index[32];
        std::snprintf(index, sizeof(index), "%06zu", i);
        rgb_files.push_back(path + "/frame-" + index + ".color.jpg");
        depth_files.push_back(path + "/frame-" + index + ".depth.png");
    }
}

void ReadImageSequenceFromScannetWithPose(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                                          std::vector<geometry::TransformationMatrix>& poses, camera::PinholeCamera& rgb_camera,
                                          camera::PinholeCamera& depth_camera) {
    ReadImageSequenceFromScannet(path, rgb_files, depth_files, rgb_camera, depth_camera);
    poses.clear();
    for (size_t i = 0; i < rgb_files.size(); ++i) {
        char index[32];
        std::snprintf(index, sizeof(index), "%06zu", i);
        std::ifstream pose_in((path + "/frame-" + index + ".pose.txt").c_str());
        geometry::TransformationMatrix T;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) pose_in >> T(r, c);
        poses.push_back(T);
    }
}

} // namespace tool
} // namespace one_piece
