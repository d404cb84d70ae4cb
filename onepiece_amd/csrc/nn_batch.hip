// nn_batch.hip -- batches of exact nearest-neighbour queries against one target cloud, and the label transfer built on them: what
// example/GetLabelUsingKDTree.cpp does with one KDTree<>::KnnSearch(q, ..., 1) per vertex (Geometry/KDTree.h:147-196) followed by
// `dists[0] < max_distance`.  An index is built once over the target (the example queries the annotated mesh for its semantic and for its
// instance pass) and answers any number of batches.
//
// The search structure is the registration path's (icp_core.hpp / icp_grid.hip: Grid, cell_coord, bounding box -> cell counts -> scan ->
// counting sort into float4 records); only the cell size differs -- it follows the target's density (icp_create's comment), not a
// threshold: ICP's `cell = threshold`, 27-cell form would put thousands of mesh vertices into a 0.316 m cell.
//
// Per batch:
//   k_nn_check    one lane per query: non-finite coordinates set an error word (the batch is refused: nanoflann's answer to such a query
//                 is an artefact of its traversal, and the class surface's host loop produces it)
//   the counting sort of icp_grid.hip over the QUERIES on the target's grid (cell_sort_points).  Queries are mesh vertices in file order:
//                 neighbouring lanes would walk unrelated cells, every candidate load its own cache line and every wave as long as its
//                 unluckiest lane.  Sorted, a wave's lanes share their cells (one fetch serves them all) and stop after the same ring.  The
//                 sort is three small launches over tables the size of the grid; results go back by the original index the record carries.
//   k_nn_query    one lane per sorted query: rings of cells around the query's cell, nearest candidate by the unsigned minimum over
//                 (distance bits, index) keys and the runner-up's distance, until the answer is provably final (below)
//   the host      re-decides the reported queries in op_host::NanoTree (the tree nanoflann 1.3.2 would build), k_nn_patch puts the answers in
//   k_nn_gather   out[i] = idx[i] >= 0 ? labels[idx[i]] : default_label
//
// The distance is nanoflann's L2_Simple_Adaptor in float32: d = 0; d += dx*dx; d += dy*dy; d += dz*dz -- every product and every sum rounded
// on its own (the unit is built with -ffp-contract=off), dx = q - p.
//
// WHEN THE SCAN MAY STOP.  After ring r the cells [c - r, c + r]^3 have been read.  A target that has not been read lies, along some axis,
// in a cell K >= c + r + 1 or K <= c - r - 1.  Cells come from cell_coord: fl(fl(p - o) * inv) >= K, two roundings of relative size 2^-24
// each, hence p - o >= K * cell * (1 - 2^-23) with cell = 1 / inv, and likewise p - o < (K + 1) * cell * (1 + 2^-23) on the low side (clamping
// only moves a point to a cell nearer the box, which keeps both inequalities).  The kernel evaluates the face distances
//     (c + r + 1) * cell * (1 - 2^-22) - (q - o)      and      (q - o) - (c - r) * cell * (1 + 2^-22)
// in double (q, o, inv are floats: differences and products carry 2^-53 at most); what lies behind a face also lies inside the grid's
// box, 0 <= p - o < g * cell * (1 + 2^-23), so a query outside the box adds its squared distance to the box along the OTHER two axes (a query
// far away is done after the ring that holds its nearest target, not after the whole grid).  The smallest such sum over the faces that still
// have cells behind them, times (1 - 2^-20), is reach2; no such face: everything has been read.  The float distance of an unread point is at
// least its real squared distance times (1 - 2^-21) (the rounding of q - p, of each product and of each sum), so it is ABOVE reach2.
// The scan stops when  best * (1 + kDoubtRel) < reach2:  nothing unread can beat, tie or come within the doubt margin of the best.  With a finite cutoff it also stops when  reach2 >= max_sq_dist * (1 + kDoubtRel):  nothing unread
// is below the cutoff, or within the doubt margin of a best that is.  The query's own cell only says where the rings are centred: a
// query outside the box is clamped to the nearest cell and the same inequalities hold, with faces that are far away.
//
// AGREEMENT WITH THE TREE.  nanoflann's knnSearch(…, 1) does not always return the minimum over (distance, index):
//   * among exactly equidistant points it keeps the one its traversal meets first;
//   * it skips a branch when its float lower bound exceeds the best so far, and that bound is a chain: bound = bound + cut - kept per level
//     (onepiece_nanotree.hpp, descend()).  Along a root-to-node path the bound only grows (cut >= kept: the cells are nested), so every
//     intermediate is at most 2 B for the final bound B; a level rounds fl(bound + cut) (<= 2^-24 * 2 B), the subtraction (<= 2^-24 * B) and
//     cut = fl(fl(v - c)^2) (<= 2 * 2^-24 * B): 5 * 2^-24 * B per level.  The candidates' own distances carry 4 * 2^-24 against the real
//     ones.  So a branch can be skipped wrongly only if it holds a point within (5 * depth + 4) * 2^-24, relatively, of the best found.
//     kDoubtRel = 2^-15 = 512 * 2^-24 covers a depth of 101 levels; a tree over 2^28 points with leaves of 10 is 25 levels deep when
//     balanced, and the middle split of a cell cannot halve a float interval more than a few dozen times per axis.
// Both cases are reported by the kernel -- runner-up equal to the best (`tied`), or within kDoubtRel of it (`doubtful`) -- and re-decided on
// the host in the tree itself; every other query's answer is the unique minimum, which the tree must return too.  On uniform random clouds the
// chance of a runner-up within kDoubtRel is ~1.5 * kDoubtRel per query (volumes of the two nearest balls): none or one in thousands.
#include <thread>

#include "icp_core.hpp"

namespace {

using op::check_mem;
using op::Scope;

constexpr int kNnThreads = 256;
constexpr float kDoubtRel = 1.0f / 32768.0f;   // 2^-15 (derivation above)
// Targets per occupied cell the grid is sized for.  A query reads at least its own cell and usually the ring around it (up to 27 cells):
// ~10 a cell keeps that at a few hundred candidates while the cell table stays a tenth of the target's size.  NOT MEASURED on the device
// yet; the value is k_estimate_normals' experience (a first ring that holds a few times the neighbours asked for) applied to k = 1.
constexpr double kPointsPerCell = 10.0;
constexpr size_t kHostThreadsFrom = 4096;      // reported queries from which the host re-decides them on several threads (the tree is finished first)

__global__ __launch_bounds__(kNnThreads) void k_nn_check(const float* __restrict__ xyz, size_t n, unsigned* __restrict__ bad) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) atomicOr(bad, 1u);
}

struct NnReport { unsigned tied, doubtful, listed, pad; };

__global__ __launch_bounds__(kNnThreads) void k_nn_query(Grid g, const unsigned* __restrict__ cell_start, const float4* __restrict__ tgt,
                                                         const float4* __restrict__ queries /* cell-sorted, .w = original index */, size_t n,
                                                         float max_sq_dist, int* __restrict__ out_idx, float* __restrict__ out_dist,
                                                         NnReport* __restrict__ report, unsigned* __restrict__ list) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 me = queries[i];
    const int cx = cell_coord(me.x, g.ox, g.inv_cell, g.gx), cy = cell_coord(me.y, g.oy, g.inv_cell, g.gy),
              cz = cell_coord(me.z, g.oz, g.inv_cell, g.gz);
    unsigned long long best = kNoKey;   // (FLT_MAX, 0): a candidate at FLT_MAX or beyond is no answer, as in nanoflann (its worst distance starts there)
    float second = FLT_MAX;
    const double cell = 1.0 / (double)g.inv_cell;
    const double qx = (double)me.x - (double)g.ox, qy = (double)me.y - (double)g.oy, qz = (double)me.z - (double)g.oz;
    const double up = 1.0 + 0x1p-22, down = 1.0 - 0x1p-22;
    const double cut2 = (double)max_sq_dist * (1.0 + (double)kDoubtRel); // inf for no cutoff
    // how far the query lies outside the grid's box along each axis, squared (0 inside): every target has 0 <= p - o < g * cell * (1 + 2^-23)
    auto outside = [&](double q, int cells) __attribute__((always_inline)) { const double d = fmax(0.0, fmax(-q, q - (double)cells * cell * up)); return d * d; };
    const double off_x = outside(qx, g.gx), off_y = outside(qy, g.gy), off_z = outside(qz, g.gz);
    auto behind = [&](double gap, double others) __attribute__((always_inline)) { gap = fmax(gap, 0.0); return gap * gap + others; };
    const int max_ring = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
    for (int ring = 0; ring <= max_ring; ++ring) {
        const int z_lo = max(cz - ring, 0), z_hi = min(cz + ring, g.gz - 1), y_lo = max(cy - ring, 0), y_hi = min(cy + ring, g.gy - 1);
        for (int z = z_lo; z <= z_hi; ++z)
            for (int y = y_lo; y <= y_hi; ++y) {
                const bool shell_row = (z == cz - ring || z == cz + ring || y == cy - ring || y == cy + ring);
                // on a shell row the whole x run, otherwise only the two x end cells of the ring
                for (int part = 0; part < (shell_row || ring == 0 ? 1 : 2); ++part) {
                    int x_lo, x_hi;
                    if (shell_row) { x_lo = cx - ring; x_hi = cx + ring; }
                    else x_lo = x_hi = part == 0 ? cx - ring : cx + ring;
                    x_lo = max(x_lo, 0); x_hi = min(x_hi, g.gx - 1);
                    if (x_lo > x_hi) continue;
                    const size_t row = ((size_t)z * g.gy + y) * g.gx;
                    const unsigned beg = cell_start[row + x_lo], end = cell_start[row + x_hi + 1]; // the table has ncell + 4 entries
                    for (unsigned p = beg; p < end; p += 4) { // four candidates in flight per trip
                        float4 c[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) c[k] = tgt[min(p + k, end - 1)];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (p + k >= end) continue;
                            const float dx = me.x - c[k].x, dy = me.y - c[k].y, dz = me.z - c[k].z;
                            float d = 0.0f;
                            d += dx * dx; d += dy * dy; d += dz * dz;
                            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(c[k].w);
                            if (key < best) { second = __uint_as_float((unsigned)(best >> 32)); best = key; }
                            else if (d < second) second = d;
                        }
                    }
                }
            }
        double reach2 = HUGE_VAL; // squared distance to the nearest face that still has cells behind it, the query's distance to the box along the other axes included
        if (cx - ring > 0) reach2 = fmin(reach2, behind(qx - (double)(cx - ring) * cell * up, off_y + off_z));
        if (cx + ring < g.gx - 1) reach2 = fmin(reach2, behind((double)(cx + ring + 1) * cell * down - qx, off_y + off_z));
        if (cy - ring > 0) reach2 = fmin(reach2, behind(qy - (double)(cy - ring) * cell * up, off_x + off_z));
        if (cy + ring < g.gy - 1) reach2 = fmin(reach2, behind((double)(cy + ring + 1) * cell * down - qy, off_x + off_z));
        if (cz - ring > 0) reach2 = fmin(reach2, behind(qz - (double)(cz - ring) * cell * up, off_x + off_y));
        if (cz + ring < g.gz - 1) reach2 = fmin(reach2, behind((double)(cz + ring + 1) * cell * down - qz, off_x + off_y));
        if (reach2 == HUGE_VAL) break; // no cell left behind any face
        reach2 *= 1.0 - 0x1p-20;
        if (best != kNoKey && (double)__uint_as_float((unsigned)(best >> 32)) * (1.0 + (double)kDoubtRel) < reach2) break;
        if (reach2 >= cut2) break;
    }
    const unsigned orig = __float_as_uint(me.w);
    const float bd = __uint_as_float((unsigned)(best >> 32));
    const bool found = best != kNoKey;
    const bool matched = found && bd < max_sq_dist; // strict, as `dists[0] < max_distance`
    out_idx[orig] = matched ? (int)(unsigned)(best & 0xffffffffull) : -1;
    out_dist[orig] = matched ? bd : __uint_as_float(0x7f800000u);
    // runner-up equal to the best, or within the margin of the tree's bound chain: the tree decides (also between a best below the cutoff and a runner-up beyond it)
    if (found && second <= bd + bd * kDoubtRel) {
        atomicAdd(second == bd ? &report->tied : &report->doubtful, 1u);
        list[atomicAdd(&report->listed, 1u)] = orig; // every query reports at most once: listed <= n
    }
}

struct NnPatch { unsigned query; int idx; float dist; };

__global__ __launch_bounds__(kNnThreads) void k_nn_patch(const NnPatch* __restrict__ patch, size_t count, int* __restrict__ idx, float* __restrict__ dist) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const NnPatch p = patch[i];
    idx[p.query] = p.idx;
    dist[p.query] = p.dist;
}

__global__ __launch_bounds__(kNnThreads) void k_nn_gather(const int* __restrict__ idx, size_t n, const int* __restrict__ labels, size_t m, int default_label,
                                                          int* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = idx[i];
    out[i] = t >= 0 && (size_t)t < m ? labels[t] : default_label;
}

__global__ __launch_bounds__(kNnThreads) void k_nn_fill(int* __restrict__ idx, float* __restrict__ dist, int* __restrict__ labels, size_t n, int default_label) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (idx) idx[i] = -1;
    if (dist) dist[i] = __uint_as_float(0x7f800000u);
    if (labels) labels[i] = default_label;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kNnThreads - 1) / kNnThreads); }

inline bool all_finite(const float* v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!(std::fabs(v[i]) <= FLT_MAX)) return false;
    return true;
}

} // namespace

struct op_nn_index {
    int device = 0;
    size_t m = 0;
    op_icp* ctx = nullptr;             // the target, its grid and its cell-sorted records (icp_grid.hip); null for an empty target
    std::vector<float> tgt_host;       // the target in original order: what the tree searches
    op_host::NanoTree tree;            // laid down at the first reported query, split where searches go, finished before threads share it
    bool tree_finished = false;
    uint64_t queries = 0, tied = 0, doubtful = 0;
};

namespace {

// the host's part: every listed query is answered by the tree; -> patches (cutoff applied)
void redecide(op_nn_index* ix, const float* q_host, const unsigned* list, size_t count, float max_sq_dist, std::vector<NnPatch>& patch) {
    if (!ix->tree.built()) ix->tree.build(ix->tgt_host.data(), ix->m, 10, false);
    patch.resize(count);
    auto one = [&](size_t k) {
        const unsigned qi = list[k];
        const float* q = q_host + 3 * (size_t)qi;
        const int t = ix->tree.nearest(q);
        float d = 0.0f;
        if (t >= 0) {
            const float* p = ix->tgt_host.data() + 3 * (size_t)t;
            for (int c = 0; c < 3; ++c) { const float diff = q[c] - p[c]; d += diff * diff; }
        }
        const bool matched = t >= 0 && d < max_sq_dist;
        patch[k].query = qi;
        patch[k].idx = matched ? t : -1;
        patch[k].dist = matched ? d : std::numeric_limits<float>::infinity();
    };
    if (count < kHostThreadsFrom) {
        for (size_t k = 0; k < count; ++k) one(k);
        return;
    }
    if (!ix->tree_finished) { ix->tree.finish(); ix->tree_finished = true; } // splitting is not thread-safe; searching a finished tree is
    const unsigned workers = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < workers; ++w)
        pool.emplace_back([&, w]() { for (size_t k = w; k < count; k += workers) one(k); });
    for (std::thread& t : pool) t.join();
}

// queries -> indices (and distances, labels) in device buffers of the scope; outputs follow `mem`
int nn_query(op_nn_index* ix, const int* tgt_labels, const float* query_xyz, size_t n, int mem, float max_sq_dist, int default_label, int* out_idx,
             float* out_sq_dist, int* out_labels) {
    if (!ix) return fail(OP_ERR_INVALID, "null index");
    OP_TRY(check_mem(mem));
    if (n == 0) return OP_OK;
    if (!query_xyz || (!out_idx && !out_labels) || (out_labels && !tgt_labels && ix->m)) return fail(OP_ERR_INVALID, "null argument");
    if (max_sq_dist != max_sq_dist) return fail(OP_ERR_INVALID, "max_sq_dist is NaN");
    if (n >= kMaxPoints) return fail(OP_ERR_INVALID, "too many queries (at most %zu)", kMaxPoints - 1);
    Scope s;
    OP_TRY(s.open(ix->device));
    int* d_idx = nullptr;
    float* d_dist = nullptr;
    int* d_out_labels = nullptr;
    if (mem == OP_MEM_DEVICE && out_idx) d_idx = out_idx; else OP_TRY(s.alloc(&d_idx, n));
    if (mem == OP_MEM_DEVICE && out_sq_dist) d_dist = out_sq_dist; else OP_TRY(s.alloc(&d_dist, n));
    if (out_labels) { if (mem == OP_MEM_DEVICE) d_out_labels = out_labels; else OP_TRY(s.alloc(&d_out_labels, n)); }
    const float* d_q = nullptr;
    OP_TRY(s.input(query_xyz, n * 3, mem, &d_q));
    unsigned* d_bad = nullptr;   // [0] the error word, then the report
    OP_TRY(s.alloc(&d_bad, (size_t)8));
    OP_HIP(hipMemsetAsync(d_bad, 0, 8 * sizeof(unsigned), s.stream));
    hipLaunchKernelGGL(k_nn_check, dim3(blocks_for(n)), dim3(kNnThreads), 0, s.stream, d_q, n, d_bad);
    OP_HIP(hipGetLastError());
    unsigned bad = 0;
    OP_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    if (bad) return fail(OP_ERR_INVALID, "a query coordinate is not finite");
    if (ix->m == 0) { // nothing to find: -1 and the default label everywhere
        hipLaunchKernelGGL(k_nn_fill, dim3(blocks_for(n)), dim3(kNnThreads), 0, s.stream, d_idx, d_dist, d_out_labels, n, default_label);
        OP_HIP(hipGetLastError());
    } else {
        op_icp* c = ix->ctx;
        float4* d_sorted = nullptr;
        OP_TRY(s.alloc(&d_sorted, n));
        OP_TRY(cell_sort_points(d_q, n, c->grid, c->ncell, d_sorted, s.stream));
        NnReport* d_report = reinterpret_cast<NnReport*>(d_bad + 4);
        unsigned* d_list = nullptr;
        OP_TRY(s.alloc(&d_list, n));
        hipLaunchKernelGGL(k_nn_query, dim3(blocks_for(n)), dim3(kNnThreads), 0, s.stream, c->grid, (const unsigned*)c->cell_start, (const float4*)c->tgt,
                           (const float4*)d_sorted, n, max_sq_dist, d_idx, d_dist, d_report, d_list);
        OP_HIP(hipGetLastError());
        NnReport report = {0, 0, 0, 0};
        OP_HIP(hipMemcpyAsync(&report, d_report, sizeof(report), hipMemcpyDeviceToHost, s.stream));
        OP_HIP(hipStreamSynchronize(s.stream));
        if (report.listed > n || report.tied + report.doubtful != report.listed) return fail(OP_ERR_HIP, "nearest-neighbour report is inconsistent");
        ix->queries += n; ix->tied += report.tied; ix->doubtful += report.doubtful;
        if (report.listed) {
            std::vector<unsigned> list(report.listed);
            OP_HIP(hipMemcpy(list.data(), d_list, list.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
            std::vector<float> q_copy;
            const float* q_host = query_xyz;
            if (mem == OP_MEM_DEVICE) {
                q_copy.resize(n * 3);
                OP_HIP(hipMemcpy(q_copy.data(), d_q, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
                q_host = q_copy.data();
            }
            std::vector<NnPatch> patch;
            redecide(ix, q_host, list.data(), list.size(), max_sq_dist, patch);
            NnPatch* d_patch = nullptr;
            OP_TRY(s.upload(patch, &d_patch));
            hipLaunchKernelGGL(k_nn_patch, dim3(blocks_for(patch.size())), dim3(kNnThreads), 0, s.stream, (const NnPatch*)d_patch, patch.size(), d_idx, d_dist);
            OP_HIP(hipGetLastError());
        }
        if (out_labels) {
            const int* d_labels = nullptr;
            OP_TRY(s.input(tgt_labels, ix->m, mem, &d_labels));
            hipLaunchKernelGGL(k_nn_gather, dim3(blocks_for(n)), dim3(kNnThreads), 0, s.stream, (const int*)d_idx, n, d_labels, ix->m, default_label, d_out_labels);
            OP_HIP(hipGetLastError());
        }
    }
    if (mem == OP_MEM_HOST) {
        if (out_idx) OP_TRY(s.output(out_idx, (const int*)d_idx, n, mem));
        if (out_sq_dist) OP_TRY(s.output(out_sq_dist, (const float*)d_dist, n, mem));
        if (out_labels) OP_TRY(s.output(out_labels, (const int*)d_out_labels, n, mem));
    }
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

} // namespace

extern "C" {

int op_nn_index_create(const float* tgt_xyz, size_t m, int mem, int device, op_nn_index** out) {
    if (!out) return fail(OP_ERR_INVALID, "null out");
    *out = nullptr;
    if (!tgt_xyz && m) return fail(OP_ERR_INVALID, "null target");
    OP_TRY(check_mem(mem));
    if (m >= kMaxPoints) return fail(OP_ERR_INVALID, "target too large (at most %zu points: the packed (distance, index) key and 32-bit record offsets)", kMaxPoints - 1);
    OP_TRY(op::use_device(device));
    op_nn_index* ix = new op_nn_index();
    ix->device = device; ix->m = m;
    ix->tgt_host.resize(m * 3);
    if (m) {
        if (mem == OP_MEM_HOST) std::memcpy(ix->tgt_host.data(), tgt_xyz, m * 3 * sizeof(float));
        else {
            const hipError_t e = hipMemcpy(ix->tgt_host.data(), tgt_xyz, m * 3 * sizeof(float), hipMemcpyDeviceToHost);
            if (e != hipSuccess) { delete ix; return fail(OP_ERR_HIP, "copy of the target failed: %s", hipGetErrorString(e)); }
        }
        if (!all_finite(ix->tgt_host.data(), m * 3)) { delete ix; return fail(OP_ERR_INVALID, "a target coordinate is not finite"); }
        const int rc = grid_context_create(tgt_xyz, m, kPointsPerCell, mem, device, &ix->ctx); // OP_ERR_INVALID for a box the grid cannot be sized for
        if (rc != OP_OK) { delete ix; return rc; }
    }
    *out = ix;
    return OP_OK;
}

int op_nn_index_destroy(op_nn_index* ix) {
    if (!ix) return OP_OK;
    if (ix->ctx) op_icp_destroy(ix->ctx);
    delete ix;
    return OP_OK;
}

int op_nn_index_query(op_nn_index* ix, const float* query_xyz, size_t n, int mem, float max_sq_dist, int32_t* out_idx, float* out_sq_dist) {
    if (n && !out_idx) return fail(OP_ERR_INVALID, "null argument");
    return nn_query(ix, nullptr, query_xyz, n, mem, max_sq_dist, 0, out_idx, out_sq_dist, nullptr);
}

int op_nn_index_transfer_labels(op_nn_index* ix, const int32_t* tgt_labels, const float* query_xyz, size_t n, int mem, float max_sq_dist,
                                int32_t default_label, int32_t* out_labels, int32_t* out_idx) {
    if (n && !out_labels) return fail(OP_ERR_INVALID, "null argument");
    return nn_query(ix, tgt_labels, query_xyz, n, mem, max_sq_dist, default_label, out_idx, nullptr, out_labels);
}

int op_nn_index_stats(op_nn_index* ix, uint64_t* queries, uint64_t* tied, uint64_t* doubtful) {
    if (!ix) return fail(OP_ERR_INVALID, "null index");
    if (queries) *queries = ix->queries;
    if (tied) *tied = ix->tied;
    if (doubtful) *doubtful = ix->doubtful;
    return OP_OK;
}

int op_transfer_labels(const float* tgt_xyz, const int32_t* tgt_labels, size_t m, const float* query_xyz, size_t n, int mem, int device, float max_sq_dist,
                       int32_t default_label, int32_t* out_labels, int32_t* out_idx) {
    op_nn_index* ix = nullptr;
    OP_TRY(op_nn_index_create(tgt_xyz, m, mem, device, &ix));
    const int rc = op_nn_index_transfer_labels(ix, tgt_labels, query_xyz, n, mem, max_sq_dist, default_label, out_labels, out_idx);
    op_nn_index_destroy(ix);
    return rc;
}

} // extern "C"
