// Tool/IO.h -- the sequence-directory readers the fusion drivers call (reference: src/Tool/IO.cpp:59-108):
// associate.txt ("t_rgb rgb_path t_depth depth_path" per line) and trajectory.txt (16 floats per line = row-major
// camera-to-world pose); the ScanNet layout (IO.cpp:109-197: _info.txt, frame-%06d.color.jpg / .depth.png / .pose.txt); and
// tool::AlignColorToDepth (IO.cpp:9-58), which re-samples the colour image of a second camera onto the depth pixels.
#pragma once
#include <string>
#include <vector>

#include "Camera/Camera.h"
#include "Geometry/Geometry.h"

namespace one_piece {
namespace tool {

void ReadImageSequence(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files);
void ReadImageSequenceWithPose(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                               std::vector<geometry::TransformationMatrix>& poses);
// color_to_depth maps depth-camera coordinates to colour-camera coordinates (the reference's name for it).  The host loop is the definition
// (DESIGN.md section 0); with OP_RUNTIME_OPT_COLOR_ALIGNMENT = 1 the call forwards to op_align_color_to_depth (bit-identical) and falls back to the
// host loop for images the device entry refuses.
cv::Mat AlignColorToDepth(const cv::Mat& color, const cv::Mat& depth, const camera::PinholeCamera& rgb_camera, const camera::PinholeCamera& depth_camera,
                          const geometry::TransformationMatrix& color_to_depth = geometry::TransformationMatrix::Identity());
void ReadImageSequenceFromScannet(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                                  camera::PinholeCamera& rgb_camera, camera::PinholeCamera& depth_camera);
void ReadImageSequenceFromScannetWithPose(const std::string& path, std::vector<std::string>& rgb_files, std::vector<std::string>& depth_files,
                                          std::vector<geometry::TransformationMatrix>& poses, camera::PinholeCamera& rgb_camera,
                                          camera::PinholeCamera& depth_camera);

} // namespace tool
} // namespace one_piece
