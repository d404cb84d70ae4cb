// Geometry/KDTree.h -- geometry::KDTree<T> and geometry::SearchParameter (reference: src/Geometry/KDTree.h:12-259, the NANO_IMPLAMENTATION
// branch: nanoflann 1.3.2 behind a thin wrapper).  A host-side structure in the reference and here.  The searches run over the tree
// nanoflann would build from the same points (../../include/onepiece_nanotree.hpp), so results agree with the reference's index for
// index: order of a k-NN list, the pick among exactly equidistant points, and which neighbours a capped radius search stops at.
//
// As in the reference: distances in and out are SQUARED L2 (`dists`, and `radius` is compared with them as given -- KDTree.h:133,248-252);
// SearchParameter::checks is accepted and ignored (nanoflann ignores it too), KnnSearch / KnnRadiusSearch use nanoflann's default search
// parameters (eps = 0) whatever `sp` says, RadiusSearch passes sp.eps and sp.sorted on and collects at most 2.5 x max_result neighbours
// before keeping the first max_result of them.
//
// EXTENSION (not in the reference): NearestBatch, the loop of KnnSearch(q, ..., 1) + cutoff that example/GetLabelUsingKDTree.cpp writes three
// times, as one call -- so that OP_RUNTIME_OPT_NEAREST_BATCH = 1 can hand the whole batch to the device (op_nn_index_query).
#pragma once
#include <algorithm>
#include <iostream>
#include <limits>
#include <utility>
#include <vector>
#include "Geometry/Geometry.h"
#include "Tool/ConsoleColor.h"
#include "onepiece_nanotree.hpp"

namespace one_piece {
namespace geometry {

class SearchParameter {
public:
    SearchParameter(int _checks = 256, float _eps = 1e-8, bool _sorted = true) {
        checks = _checks;
        eps = _eps;
        sorted = _sorted;
    }
    bool sorted = true;
    float eps = 1e-8;
    int checks = 32;
};

namespace detail {
// The device side of KDTree<3>::NearestBatch lives in the class library (src/NearestBatch.cpp), which installs these three functions when it is
// loaded; this header stays usable on its own (a program that includes it and links nothing gets the host loop).  `index` is the tree's op_nn_index,
// created on the first batch; query() returning false = the option is off or the device entry refused the input, and the caller runs its host loop.
struct NearestHooks {
    bool (*query)(void*& index, const float* targets, size_t m, const float* queries, size_t n, float max_sq_dist, int* indices, float* dists);
    void (*drop)(void*& index);
    void (*stats)(void* index, unsigned long long& queries, unsigned long long& tied, unsigned long long& doubtful);
};
inline NearestHooks& Hooks() { static NearestHooks hooks = {nullptr, nullptr, nullptr}; return hooks; }
inline bool NearestBatchOnDevice(void*& index, const float* targets, size_t m, const float* queries, size_t n, float max_sq_dist, int* indices, float* dists) {
    return Hooks().query && Hooks().query(index, targets, m, queries, n, max_sq_dist, indices, dists);
}
inline void DropNearestIndex(void*& index) {
    if (index && Hooks().drop) Hooks().drop(index);
    index = nullptr;
}
inline void NearestIndexStats(void* index, unsigned long long& queries, unsigned long long& tied, unsigned long long& doubtful) { // zeros without an index
    queries = tied = doubtful = 0;
    if (index && Hooks().stats) Hooks().stats(index, queries, tied, doubtful);
}
} // namespace detail

template <int T = 3>
class KDTree {
public:
    KDTree(int _max_leaf = 10) : max_leaf(_max_leaf) {}
    // a copy searches the same points but owns no device index: it creates its own on its first batch
    KDTree(const KDTree& o) : tree(o.tree), flat(o.flat), max_leaf(o.max_leaf) {}
    KDTree& operator=(const KDTree& o) {
        if (this != &o) { detail::DropNearestIndex(device_index); tree = o.tree; flat = o.flat; max_leaf = o.max_leaf; }
        return *this;
    }
    ~KDTree() { detail::DropNearestIndex(device_index); }

    void BuildTree(const geometry::PointXList& points) {
        flat.resize(points.size() * (size_t)T);
        for (size_t i = 0; i != points.size(); ++i) {
            if (points[i].rows() != T) {
                std::cout << RED << "[ERROR]::[BuildKDTree]::The dimension of point is not equal to the dimension of kdtree." << RESET << std::endl;
                detail::DropNearestIndex(device_index);
                flat.clear();
                tree.build(nullptr, 0, (size_t)max_leaf);
                return;
            }
            for (int d = 0; d < T; ++d) flat[i * (size_t)T + d] = points[i](d);
        }
        detail::DropNearestIndex(device_index);
        tree.build(flat.data(), points.size(), (size_t)max_leaf);
    }
    void BuildTree(const geometry::PointList<T>& points) {
        flat.resize(points.size() * (size_t)T);
        for (size_t i = 0; i != points.size(); ++i)
            for (int d = 0; d < T; ++d) flat[i * (size_t)T + d] = points[i](d);
        detail::DropNearestIndex(device_index);
        tree.build(flat.data(), points.size(), (size_t)max_leaf);
    }

    // EXTENSION (not in the reference): for every query the index of its nearest point and the squared distance, as KnnSearch(q, indices, dists, 1)
    // reports them, kept only when `dists[0] < max_sq_dist` (strict, example/GetLabelUsingKDTree.cpp:56); otherwise -1 and +infinity.
    // OP_RUNTIME_OPT_NEAREST_BATCH = 0 (default): that loop.  1, for T = 3: the batch goes to op_nn_index_query over an index that is created on the
    // first batch and dropped by BuildTree -- the same indices and distance bits; input the device entry refuses takes the loop.
    void NearestBatch(const geometry::PointList<T>& queries, std::vector<int>& indices, std::vector<float>& dists,
                      float max_sq_dist = std::numeric_limits<float>::infinity()) {
        const size_t n = queries.size();
        indices.assign(n, -1);
        dists.assign(n, std::numeric_limits<float>::infinity());
        if (!n) return;
        if (T == 3 && tree.built()) {
            static_assert(sizeof(geometry::Vector<T>) == T * sizeof(float), "PointList must be a contiguous float array");
            if (detail::NearestBatchOnDevice(device_index, flat.data(), tree.size(), queries[0].data(), n, max_sq_dist, indices.data(), dists.data())) return;
            indices.assign(n, -1);
            dists.assign(n, std::numeric_limits<float>::infinity());
        }
        for (size_t i = 0; i < n; ++i) {
            size_t found = 0;
            float d = 0;
            if (tree.knn(queries[i].data(), 1, &found, &d) && d < max_sq_dist) { indices[i] = static_cast<int>(found); dists[i] = d; }
        }
    }

    // The reference spells every search out four times (dynamic / fixed-size query x int / size_t indices); here the twelve public overloads
    // forward to three private templates.
    // ---- RadiusSearch (KDTree.h:99-146)
    void RadiusSearch(const geometry::VectorX& point, std::vector<int>& indices, std::vector<float>& dists, double radius, size_t max_result,
                      const SearchParameter& sp = SearchParameter()) { WithinRadius(point, indices, dists, radius, max_result, sp, "[ERROR]::[RadiusSearch]::Wrong dimension!"); }
    void RadiusSearch(const geometry::VectorX& point, std::vector<size_t>& indices, std::vector<float>& dists, double radius, size_t max_result,
                      const SearchParameter& sp = SearchParameter()) { WithinRadius(point, indices, dists, radius, max_result, sp, "[ERROR]::[RadiusSearch]::Wrong dimension!"); }
    void RadiusSearch(const geometry::Vector<T>& point, std::vector<int>& indices, std::vector<float>& dists, double radius, size_t max_result,
                      const SearchParameter sp = SearchParameter()) { WithinRadius(point, indices, dists, radius, max_result, sp, nullptr); }
    void RadiusSearch(const geometry::Vector<T>& point, std::vector<size_t>& indices, std::vector<float>& dists, double radius, size_t max_result,
                      const SearchParameter sp = SearchParameter()) { WithinRadius(point, indices, dists, radius, max_result, sp, nullptr); }

    // ---- KnnSearch (KDTree.h:147-196); the reference calls knnSearch with nanoflann's default parameters whatever `sp` says
    void KnnSearch(const geometry::VectorX& point, std::vector<int>& indices, std::vector<float>& dists, int k, const SearchParameter& sp = SearchParameter()) {
        (void)sp; Nearest(point, indices, dists, k, "[ERROR]::[KnnSearch]::Wrong dimension!");
    }
    void KnnSearch(const geometry::VectorX& point, std::vector<size_t>& indices, std::vector<float>& dists, int k, const SearchParameter& sp = SearchParameter()) {
        (void)sp; Nearest(point, indices, dists, k, "[ERROR]::[KnnSearch]::Wrong dimension!");
    }
    void KnnSearch(const geometry::Vector<T>& point, std::vector<int>& indices, std::vector<float>& dists, int k, const SearchParameter& sp = SearchParameter()) {
        (void)sp; Nearest(point, indices, dists, k, nullptr);
    }
    void KnnSearch(const geometry::Vector<T>& point, std::vector<size_t>& indices, std::vector<float>& dists, int k, const SearchParameter& sp = SearchParameter()) {
        (void)sp; Nearest(point, indices, dists, k, nullptr);
    }

    // ---- KnnRadiusSearch (KDTree.h:197-255): the k nearest, then the prefix whose squared distance does not exceed `radius`
    void KnnRadiusSearch(const geometry::VectorX& point, std::vector<int>& indices, std::vector<float>& dists, int k, float radius,
                         const SearchParameter& sp = SearchParameter()) { (void)sp; if (Nearest(point, indices, dists, k, "[ERROR]::[KnnSearch]::Wrong dimension!")) CutAt(radius, indices, dists); }
    void KnnRadiusSearch(const geometry::VectorX& point, std::vector<size_t>& indices, std::vector<float>& dists, int k, float radius,
                         const SearchParameter& sp = SearchParameter()) { (void)sp; if (Nearest(point, indices, dists, k, "[ERROR]::[KnnSearch]::Wrong dimension!")) CutAt(radius, indices, dists); }
    void KnnRadiusSearch(const geometry::Vector<T>& point, std::vector<int>& indices, std::vector<float>& dists, int k, float radius,
                         const SearchParameter& sp = SearchParameter()) { (void)sp; if (Nearest(point, indices, dists, k, nullptr)) CutAt(radius, indices, dists); }
    void KnnRadiusSearch(const geometry::Vector<T>& point, std::vector<size_t>& indices, std::vector<float>& dists, int k, float radius,
                         const SearchParameter& sp = SearchParameter()) { (void)sp; if (Nearest(point, indices, dists, k, nullptr)) CutAt(radius, indices, dists); }

    // EXTENSION (not in the reference): since the device index of NearestBatch was created -- queries it answered, and how many of them the host
    // re-decided in the tree because the runner-up was exactly as near as the best (tied) or within rounding of the tree's bound (doubtful)
    void NearestBatchStats(unsigned long long& queries, unsigned long long& tied, unsigned long long& doubtful) const {
        detail::NearestIndexStats(device_index, queries, tied, doubtful);
    }

protected:
    // the query as T floats; a dynamic vector of another length is refused with the reference's message (and the outputs are left alone, as there)
    template <class Query>
    bool Coordinates(const Query& point, float* q, const char* complaint) const {
        if (complaint && (int)point.rows() != T) {
            std::cout << RED << complaint << RESET << std::endl;
            return false;
        }
        for (int d = 0; d < T; ++d) q[d] = point(d);
        return true;
    }
    template <class Query, class Index>
    bool Nearest(const Query& point, std::vector<Index>& indices, std::vector<float>& dists, int k, const char* complaint) const {
        float q[T];
        if (!Coordinates(point, q, complaint)) return false;
        const size_t want = k > 0 ? (size_t)k : 0;
        std::vector<size_t> found(want);
        std::vector<float> d2(want);
        const size_t n = want ? tree.knn(q, want, found.data(), d2.data()) : 0;
        indices.resize(n);
        dists.resize(n);
        for (size_t i = 0; i < n; ++i) { indices[i] = static_cast<Index>(found[i]); dists[i] = d2[i]; }
        return true;
    }
    // at most 2.5 x max_result neighbours are collected (in traversal order, then sorted if asked), the first max_result of them kept
    template <class Query, class Index>
    void WithinRadius(const Query& point, std::vector<Index>& indices, std::vector<float>& dists, double radius, size_t max_result, const SearchParameter& sp,
                      const char* complaint) const {
        float q[T];
        if (!Coordinates(point, q, complaint)) return;
        std::vector<std::pair<size_t, float> > matches;
        const size_t n = std::min(tree.radius(q, static_cast<float>(radius), matches, static_cast<size_t>(max_result * 2.5), sp.eps, sp.sorted), max_result);
        indices.resize(n);
        dists.resize(n);
        for (size_t i = 0; i < n; ++i) { indices[i] = static_cast<Index>(matches[i].first); dists[i] = matches[i].second; }
    }
    template <class Index>
    static void CutAt(float radius, std::vector<Index>& indices, std::vector<float>& dists) {
        size_t keep = 0;
        while (keep != dists.size() && !(dists[keep] > radius)) ++keep;
        indices.resize(keep);
        dists.resize(keep);
    }

    void* device_index = nullptr; // op_nn_index of NearestBatch (T = 3, OP_RUNTIME_OPT_NEAREST_BATCH = 1)
    op_host::NanoTreeT<T> tree;
    std::vector<float> flat; // the points, T floats each (nanoflann's dataset adaptor reads the caller's list; here they are copied once)
    int max_leaf = 10;
};

} // namespace geometry
} // namespace one_piece
