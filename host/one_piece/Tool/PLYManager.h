// Tool/PLYManager.h -- tool::ReadPLY / tool::WritePLY with additional per-vertex properties and tool::AdditionalElement (reference:
// src/Tool/PLYManager.h:11-32, over tinyply), as example/GetLabelUsingKDTree.cpp uses them: `element_key = "vertex"`, ONE scalar property
// (char, uchar, short, ushort, int, uint or float) per AdditionalElement -- ScanNet's `label`.  Own implementation next to the other PLY code
// (src/MeshIO.cpp); tinyply::Type is the small enum below, so that `additional_labels[0].type == tinyply::Type::UINT16` reads as it does there.
// List properties and elements other than "vertex" are refused with a message.
//
// ReadPLY fills count, byte_size, type and data of every AdditionalElement whose property the file has; data is allocated with new[] and belongs
// to the caller (the example deletes it).  An element whose property is missing keeps type = INVALID, count = 0, data = nullptr.
// WritePLY writes data[0 .. count * size of type) after the standard vertex properties, binary little endian or ascii.
//
// EXTENSION (not in the reference): tool::TransferLabels, the label loop of that example as one call (Geometry/KDTree.h, NearestBatch).
#pragma once
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Tool/ConsoleColor.h"

namespace tinyply {
enum class Type { INVALID, INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 };
}

namespace one_piece {
namespace tool {

struct AdditionalElement {
    size_t count = 0;
    size_t byte_size = 0;
    std::string element_key;
    std::vector<std::string> element_property;
    tinyply::Type type = tinyply::Type::INVALID;
    tinyply::Type list_type = tinyply::Type::INVALID;
    size_t list_count = 0;
    unsigned char* data = nullptr;
};

bool ReadPLY(const std::string& filename, geometry::Point3List& points, geometry::Point3List& normals, geometry::Point3List& colors,
             geometry::Point3uiList& triangles, std::vector<AdditionalElement>& additional_labels);

bool WritePLY(const std::string& filename, const geometry::Point3List& points, const geometry::Point3List& normals, const geometry::Point3List& colors,
              const geometry::Point3uiList& triangles = geometry::Point3uiList(), const std::vector<std::string>& comments = std::vector<std::string>(),
              const std::vector<AdditionalElement>& additional_labels = std::vector<AdditionalElement>(), bool use_ascii = false);

// EXTENSION (not in the reference): out_labels[i] = the label of the target point nearest to query i when its squared distance is below max_sq_dist
// (strict), default_label otherwise -- example/GetLabelUsingKDTree.cpp:45-60.  OP_RUNTIME_OPT_NEAREST_BATCH = 0 (default): a KDTree<> and the
// loop of KnnSearch(q, ..., 1); 1: op_transfer_labels, and the loop for input the device entry refuses.  The unsigned short overload is the
// example's semantic pass: labels are widened to int for the call and narrowed back.
void TransferLabels(const geometry::Point3List& target_points, const std::vector<int>& target_labels, const geometry::Point3List& query_points,
                    float max_sq_dist, int default_label, std::vector<int>& out_labels);
void TransferLabels(const geometry::Point3List& target_points, const std::vector<unsigned short>& target_labels, const geometry::Point3List& query_points,
                    float max_sq_dist, unsigned short default_label, std::vector<unsigned short>& out_labels);

} // namespace tool
} // namespace one_piece
