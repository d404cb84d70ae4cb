// NearestBatch.cpp -- the device side of geometry::KDTree<3>::NearestBatch and tool::TransferLabels (OP_RUNTIME_OPT_NEAREST_BATCH = 1).
#include "Bridge.h"
#include "Geometry/KDTree.h"
#include "Tool/PLYManager.h"

namespace one_piece {
namespace bridge {
// OP_RUNTIME_OPT_NEAREST_BATCH: 1 = KDTree<3>::NearestBatch and tool::TransferLabels forward to op_nn_index_query / op_transfer_labels
inline bool DeviceNearestBatch() {
    long long v = 0;
    return op_runtime_get_option(OP_RUNTIME_OPT_NEAREST_BATCH, &v) == OP_OK && v == 1;
}
// input the device entry refuses takes the host loop; any other failure is reported, and the host loop still answers
inline bool Refused(int rc, const char* where) {
    if (rc == OP_ERR_INVALID || rc == OP_ERR_CAPACITY) return true;
    return Failed(rc, where);
}
} // namespace bridge

namespace geometry {
namespace {

bool QueryOnDevice(void*& index, const float* targets, size_t m, const float* queries, size_t n, float max_sq_dist, int* indices, float* dists) {
    if (!bridge::DeviceNearestBatch()) return false;
    if (!index) {
        op_nn_index* created = nullptr;
        if (bridge::Refused(op_nn_index_create(targets, m, OP_MEM_HOST, bridge::Device(), &created), "NearestBatch")) return false;
        index = created;
    }
    return !bridge::Refused(op_nn_index_query(static_cast<op_nn_index*>(index), queries, n, OP_MEM_HOST, max_sq_dist, indices, dists), "NearestBatch");
}

void DropIndex(void*& index) {
    if (index) op_nn_index_destroy(static_cast<op_nn_index*>(index));
    index = nullptr;
}

void IndexStats(void* index, unsigned long long& queries, unsigned long long& tied, unsigned long long& doubtful) {
    uint64_t q = 0, t = 0, d = 0;
    if (index) (void)op_nn_index_stats(static_cast<op_nn_index*>(index), &q, &t, &d);
    queries = q; tied = t; doubtful = d;
}

// installed when the class library is loaded (Geometry/KDTree.h, detail::NearestHooks)
const bool installed = (detail::Hooks().query = QueryOnDevice, detail::Hooks().drop = DropIndex, detail::Hooks().stats = IndexStats, true);

} // namespace
} // namespace geometry

namespace tool {

void TransferLabels(const geometry::Point3List& target_points, const std::vector<int>& target_labels, const geometry::Point3List& query_points,
                    float max_sq_dist, int default_label, std::vector<int>& out_labels) {
    out_labels.assign(query_points.size(), default_label);
    if (target_labels.size() != target_points.size()) {
        std::cout << RED << "[ERROR]::[TransferLabels]::one label per target point is needed." << RESET << std::endl;
        return;
    }
    if (query_points.empty()) return;
    if (bridge::DeviceNearestBatch()) {
        static_assert(sizeof(int) == sizeof(int32_t), "labels travel as int32");
        const int rc = op_transfer_labels(bridge::Floats(target_points), target_labels.data(), target_points.size(), bridge::Floats(query_points), query_points.size(),
                                          OP_MEM_HOST, bridge::Device(), max_sq_dist, default_label, out_labels.data(), nullptr);
        if (!bridge::Refused(rc, "TransferLabels")) return;
        out_labels.assign(query_points.size(), default_label);
    }
    geometry::KDTree<> kdtree;
    kdtree.BuildTree(target_points);
    for (size_t i = 0; i != query_points.size(); ++i) { // example/GetLabelUsingKDTree.cpp:49-60
        std::vector<int> indices;
        std::vector<float> dists;
        kdtree.KnnSearch(query_points[i], indices, dists, 1);
        if (indices.size() > 0 && dists[0] < max_sq_dist) out_labels[i] = target_labels[indices[0]];
    }
}

void TransferLabels(const geometry::Point3List& target_points, const std::vector<unsigned short>& target_labels, const geometry::Point3List& query_points,
                    float max_sq_dist, unsigned short default_label, std::vector<unsigned short>& out_labels) {
    const std::vector<int> wide(target_labels.begin(), target_labels.end());
    std::vector<int> out;
    TransferLabels(target_points, wide, query_points, max_sq_dist, static_cast<int>(default_label), out);
    out_labels.resize(out.size());
    for (size_t i = 0; i < out.size(); ++i) out_labels[i] = static_cast<unsigned short>(out[i]);
}

} // namespace tool
} // namespace one_piece
