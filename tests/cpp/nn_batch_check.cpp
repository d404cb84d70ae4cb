// nn_batch_check.cpp -- a stand-alone program (tests/test_nn_batch_cpu.py builds it with -fsanitize=address,undefined and runs it once, on the
// CPU) over the host side of the label-transfer surface: tool::WritePLY / tool::ReadPLY with an additional vertex property, and the host path of
// geometry::KDTree<>::NearestBatch against the loop of KnnSearch(q, ..., 1) + cutoff it stands for.  It is compiled together with
// host/one_piece/src/MeshIO.cpp and NearestBatch.cpp and links no device library: the handful of C-ABI entries those files name are defined
// here, with the runtime option at 0 (the host path) and the device entries unreachable.
//   nn_batch_check <scratch directory>      exit 0 = every check passed
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "Geometry/KDTree.h"
#include "Tool/PLYManager.h"
#include "src/MeshIO.h"
#include "onepiece_hip.h"
using namespace one_piece;

extern "C" {
int op_runtime_get_option(int, long long* value) { *value = 0; return OP_OK; }
int op_runtime_configure(int) { return OP_OK; }
const char* op_last_error(void) { return "no device library in this program"; }
int op_nn_index_create(const float*, size_t, int, int, op_nn_index**) { std::abort(); }
int op_nn_index_destroy(op_nn_index*) { std::abort(); }
int op_nn_index_query(op_nn_index*, const float*, size_t, int, float, int32_t*, float*) { std::abort(); }
int op_nn_index_stats(op_nn_index*, uint64_t*, uint64_t*, uint64_t*) { std::abort(); }
int op_transfer_labels(const float*, const int32_t*, size_t, const float*, size_t, int, int, float, int32_t, int32_t*, int32_t*) { std::abort(); }
}

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Rng {
    unsigned long long s;
    float Next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<float>(static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0)); }
};

bool SameBits(const geometry::Point3List& a, const geometry::Point3List& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a[0].data(), b[0].data(), a.size() * 12) == 0);
}

void CheckNearest(const geometry::Point3List& targets, const geometry::Point3List& queries, float max_sq) {
    geometry::KDTree<> tree;
    tree.BuildTree(targets);
    std::vector<int> idx;
    std::vector<float> dist;
    tree.NearestBatch(queries, idx, dist, max_sq);
    CHECK(idx.size() == queries.size() && dist.size() == queries.size());
    size_t matched = 0;
    for (size_t i = 0; i < queries.size(); ++i) {
        std::vector<int> one;
        std::vector<float> d;
        tree.KnnSearch(queries[i], one, d, 1);
        const bool keep = one.size() > 0 && d[0] < max_sq;
        CHECK(idx[i] == (keep ? one[0] : -1));
        CHECK(keep ? std::memcmp(&dist[i], &d[0], 4) == 0 : dist[i] == std::numeric_limits<float>::infinity());
        matched += keep;
    }
    if (!targets.empty() && max_sq == std::numeric_limits<float>::infinity()) CHECK(matched == queries.size());
    // a copy answers the same, and so does the tree after it has been rebuilt with other points and then with these again
    geometry::KDTree<> copy(tree);
    std::vector<int> idx2;
    copy.NearestBatch(queries, idx2, dist, max_sq);
    CHECK(idx2 == idx);
    tree.BuildTree(queries);
    tree.BuildTree(targets);
    tree.NearestBatch(queries, idx2, dist, max_sq);
    CHECK(idx2 == idx);
    unsigned long long q = 1, t = 1, dd = 1;
    tree.NearestBatchStats(q, t, dd);
    CHECK(q == 0 && t == 0 && dd == 0); // no device index on the host path
}

void CheckPly(const std::string& dir, bool ascii, bool with_attributes) {
    Rng r = {ascii ? 11ull : 12ull};
    const size_t n = 37;
    geometry::Point3List p, nrm, col;
    geometry::Point3uiList tri;
    std::vector<unsigned short> labels(n);
    for (size_t i = 0; i < n; ++i) {
        p.push_back(geometry::Point3(r.Next() * 7 - 3, r.Next() * 1e-3f, r.Next() * 1e4f));
        if (with_attributes) {
            nrm.push_back(geometry::Point3(r.Next(), -r.Next(), r.Next()));
            col.push_back(geometry::Point3(static_cast<float>(i % 256) / 255.0f, static_cast<float>((7 * i) % 256) / 255.0f, static_cast<float>(255 - i) / 255.0f));
        }
        labels[i] = static_cast<unsigned short>(i == 0 ? 65535 : (i * 977) % 41);
    }
    if (with_attributes) for (unsigned i = 0; i + 2 < n; i += 2) tri.push_back(geometry::Point3ui(i, i + 1, i + 2));
    std::vector<tool::AdditionalElement> extra(1);
    extra[0].element_key = "vertex";
    extra[0].element_property.push_back("label");
    extra[0].type = tinyply::Type::UINT16;
    extra[0].count = n;
    extra[0].byte_size = n * 2;
    extra[0].data = reinterpret_cast<unsigned char*>(labels.data());
    const std::string file = dir + (ascii ? "/check_ascii" : "/check_binary") + (with_attributes ? "_full.ply" : "_bare.ply");
    CHECK(tool::WritePLY(file, p, nrm, col, tri, std::vector<std::string>(1, "each vertex will have semantic labels."), extra, ascii));

    geometry::Point3List p2, n2, c2;
    geometry::Point3uiList t2;
    std::vector<tool::AdditionalElement> got(2);
    got[0].element_key = "vertex"; got[0].element_property.push_back("label");
    got[1].element_key = "vertex"; got[1].element_property.push_back("no_such_property");
    CHECK(tool::ReadPLY(file, p2, n2, c2, t2, got));
    CHECK(SameBits(p, p2) && SameBits(nrm, n2) && SameBits(col, c2));
    CHECK(t2.size() == tri.size() && (tri.empty() || std::memcmp(t2[0].data(), tri[0].data(), tri.size() * 12) == 0));
    CHECK(got[0].type == tinyply::Type::UINT16 && got[0].count == n && got[0].byte_size == n * 2 && got[0].data);
    if (got[0].data && got[0].byte_size == n * 2) CHECK(std::memcmp(got[0].data, labels.data(), n * 2) == 0);
    CHECK(got[1].type == tinyply::Type::INVALID && got[1].count == 0 && got[1].data == nullptr);
    delete[] got[0].data;
    // the reader behind LoadFromPLY skips the extra property
    geometry::Point3List p3, n3, c3;
    geometry::Point3uiList t3;
    CHECK(meshio::ReadPly(file, p3, n3, c3, &t3));
    CHECK(SameBits(p, p3) && SameBits(nrm, n3) && SameBits(col, c3) && t3.size() == tri.size());
    // refused: a list, another element, a count that does not fit
    std::vector<tool::AdditionalElement> bad(extra);
    bad[0].count = n - 1;
    CHECK(!tool::WritePLY(dir + "/refused.ply", p, nrm, col, tri, std::vector<std::string>(), bad, ascii));
    bad = extra; bad[0].element_key = "face";
    CHECK(!tool::WritePLY(dir + "/refused.ply", p, nrm, col, tri, std::vector<std::string>(), bad, ascii));
    bad = extra; bad[0].list_type = tinyply::Type::UINT8; bad[0].list_count = 3;
    CHECK(!tool::WritePLY(dir + "/refused.ply", p, nrm, col, tri, std::vector<std::string>(), bad, ascii));
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: nn_batch_check <scratch directory>\n"); return 2; }
    const float inf = std::numeric_limits<float>::infinity();
    Rng r = {7};
    geometry::Point3List targets, queries, lattice, halves;
    for (int i = 0; i < 700; ++i) targets.push_back(geometry::Point3(r.Next(), r.Next(), r.Next()));
    for (int i = 0; i < 450; ++i) queries.push_back(geometry::Point3(r.Next() * 1.4f - 0.2f, r.Next() * 1.4f - 0.2f, r.Next() * 1.4f - 0.2f));
    for (int rep = 0; rep < 2; ++rep)
        for (int x = 0; x < 5; ++x) for (int y = 0; y < 5; ++y) for (int z = 0; z < 5; ++z) lattice.push_back(geometry::Point3(x, y, z));
    for (int i = 0; i < 120; ++i) halves.push_back(geometry::Point3((i % 4) + 0.5f, (i / 4 % 4) + (i % 2 ? 0.5f : 0.0f), (i / 16 % 4) + (i % 3 ? 0.0f : 0.5f)));
    CheckNearest(targets, queries, inf);
    CheckNearest(targets, queries, 0.002f);
    CheckNearest(lattice, halves, inf);
    CheckNearest(lattice, halves, 0.25f); // the two-way ties sit exactly on the cutoff: strict comparison, none is matched
    CheckNearest(geometry::Point3List(), queries, inf);
    CheckNearest(targets, geometry::Point3List(), inf);
    std::vector<int> labels(targets.size()), out;
    for (size_t i = 0; i < labels.size(); ++i) labels[i] = static_cast<int>(i) - 5;
    tool::TransferLabels(targets, labels, queries, 0.002f, -7, out);
    {
        geometry::KDTree<> tree;
        tree.BuildTree(targets);
        std::vector<int> idx;
        std::vector<float> dist;
        tree.NearestBatch(queries, idx, dist, 0.002f);
        for (size_t i = 0; i < queries.size(); ++i) CHECK(out[i] == (idx[i] >= 0 ? labels[static_cast<size_t>(idx[i])] : -7));
    }
    for (int ascii = 0; ascii < 2; ++ascii)
        for (int full = 0; full < 2; ++full) CheckPly(argv[1], ascii != 0, full != 0);
    std::printf(failures ? "nn_batch_check: %d checks FAILED\n" : "nn_batch_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
