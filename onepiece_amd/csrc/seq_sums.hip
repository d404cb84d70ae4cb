// seq_sums.hip -- the sequential float32 sums of the reference-order modes (seq_sums.hpp says what they are for): the kernel k_seq_sums / k_seq_sums_many, compiled here
// once per row layout, the question whether a device may run it, the host object that takes one problem's sums (SeqSums) and the meeting of several (SeqRendezvous).
#include "seq_sums.hpp"

#include <chrono>
#include <map>

#include "common.hpp"

namespace {

constexpr int kSeqRows = 384;          // rows per tile
constexpr int kSeqStride = kSeqRows + 4; // floats between two accumulators' rows in LDS: 4 (mod 32) spreads the lanes' 16-byte reads over the banks
constexpr int kSeqProducers = 2 * kSeqRows; // 12 producer waves: producer p owns row p % kSeqRows and every second accumulator
constexpr int kSeqThreads = 1024;      // wave 0 sums; waves 4, 8 and 12 -- the ones that share its SIMD -- only keep the barriers company, the other 12 produce

// products of one row for the accumulators k = H, H + 2, ...: everything but the row's address is a compile-time constant
template <int NACC, int H>
__device__ __forceinline__ void seq_produce_row(const float* __restrict__ r, float* __restrict__ pd_row) {
    if (NACC == 42) {
        float J[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) J[i] = r[i];
#pragma unroll
        for (int k = H; k < 42; k += 2) pd_row[k * kSeqStride] = k < 36 ? J[k / 6] * J[k % 6] : J[k - 36] * J[6];
    } else {
        if (H < NACC) pd_row[H * kSeqStride] = r[H];
    }
}

// The consumer's schedule: a dependent v_add_f32 can issue every ~8 cycles, an instruction every 4 -- so the eight 16-byte LDS reads that refill one register set are
// issued one by one in the shadow of the adds that drain the other (one ds_read, then four adds: sched_group_barrier masks 0x100 = DS read, 0x2 = VALU) instead of in a
// burst in front of them, where their issue cycles add to the chain.  Measured: +2 % (ICP 586 -> 596 iterations/s, 1.4 ms of k_seq_sums per 3e5 rows either way): the
// chain itself runs at ~9.8 cycles per add in this kernel against 8.25 in the bare microbenchmark, and that is where the time is.  Scheduling only: same adds, same order.
#ifndef SEQ_NO_INTERLEAVE
#define SEQ_INTERLEAVE() do { _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) { __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x2, 4, 0); } } while (0)
#else
#define SEQ_INTERLEAVE() do { } while (0)
#endif
// Sequential float32 sums of NACC accumulators over n_pix compacted pixels of NF floats each, RPP rows per pixel.
//   NACC 42 (NF 7 * RPP): row = {J[6], r}; accumulator a*6+b += J[a]*J[b] (a, b < 6), accumulator 36+a += J[a]*r   -- the order of
//                    op_host::track_sums_reference_order: per pixel row 0 then row 1, per accumulator one rounded product and one rounded add
//   NACC 2  (NF 2):  accumulator k += value k of the pixel (NormalizeIntensity's two sums)
// One workgroup.  Wave 0 sums: lane k owns accumulator k and reads four consecutive rows of it per ds_read_b128, the next 32
// rows always in flight (two register sets) so that its only cost per row is the dependent add -- 8.25 shader cycles on this chip
// (tools/valu_ubench.hip OP 41), the floor of any sequential float32 sum; measured here: ~10 per row.  Twelve waves on the other SIMDs produce: thread p owns row
// p % 384 of the NEXT tile and every second accumulator -- 7 LDS reads, 21 multiplies, 21 LDS writes at constant offsets -- and stages
// the rows of the tile after that (global loads in flight while it multiplies).  out[0 .. NACC-1] = the sums, ((unsigned*)out)[NACC] = n_pix.
// Rows beyond the last pixel are products of zeros: acc + (+0.0f) == acc for every acc this loop can hold (it starts at +0 and a float
// sum only yields -0 from -0 + -0), so every tile is summed over all of its 384 rows.
template <int NACC, int NF, int RPP>
__device__ __forceinline__ void seq_sums_body(const float* __restrict__ rows, const unsigned* __restrict__ n_pix_ptr, float* __restrict__ out) {
    extern __shared__ float seq_lds[];
    constexpr int P = kSeqRows / RPP;                        // pixels per tile
    constexpr int RF = NF / RPP;                             // floats per row
    constexpr int kStage = P * NF;                           // floats of one staged tile
    constexpr int kLoads = (kStage + kSeqProducers - 1) / kSeqProducers;
    float* prod = seq_lds;                                   // [2][NACC][kSeqStride]
    float* stage = seq_lds + 2 * NACC * kSeqStride;          // [2][kStage]
    const unsigned n_pix = *n_pix_ptr;
    const unsigned n_tiles = (n_pix + (unsigned)P - 1u) / (unsigned)P;
    const int tid = threadIdx.x;
    const bool consumer = tid < 64;
    const int wave = tid >> 6;
    const bool idle = wave != 0 && (wave & 3) == 0;          // same SIMD as the summing wave (waves go to the SIMDs round-robin): nothing may delay its adds
    const int pj = (wave - 1 - (wave >> 2)) * 64 + (tid & 63); // producer index 0 .. 767 (meaningless for wave 0 and the idle waves)
    const int prow = pj >= kSeqRows ? pj - kSeqRows : pj;    // its row of the tile
    auto load_tile = [&](unsigned tile, float (&reg)[kLoads]) { // global -> registers (zeros beyond the data)
        const size_t base = (size_t)tile * kStage, end = (size_t)n_pix * NF;
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int e = pj + i * kSeqProducers;
            reg[i] = (e < kStage && base + (size_t)e < end) ? rows[base + (size_t)e] : 0.0f;
        }
    };
    auto store_tile = [&](int buf, const float (&reg)[kLoads]) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int e = pj + i * kSeqProducers;
            if (e < kStage) stage[buf * kStage + e] = reg[i];
        }
    };
    auto produce = [&](int buf) { // stage[buf] -> prod[buf]: RPP rows of RF floats per pixel, row * RF == pixel * NF + (row % RPP) * RF
        const float* r = stage + buf * kStage + prow * RF;
        float* pd_row = prod + buf * (NACC * kSeqStride) + prow;
        if (pj < kSeqRows) seq_produce_row<NACC, 0>(r, pd_row); // (wave-uniform: 6 waves per half)
        else seq_produce_row<NACC, 1>(r, pd_row);
    };
    float acc = 0.0f;
    float reg[kLoads];
    // prologue: tile 0 staged and produced, tile 1 staged
    const bool producer = !consumer && !idle;
    if (producer && n_tiles) { load_tile(0, reg); store_tile(0, reg); }
    __syncthreads();
    if (producer && n_tiles) { produce(0); load_tile(1, reg); store_tile(1, reg); }
    __syncthreads();
    if (consumer) __builtin_amdgcn_s_setprio(3);
    for (unsigned t = 0; t < n_tiles; ++t) {
        const int cur = (int)(t & 1u);
        if (consumer) {
            if (tid < NACC) {
                const float4* src = reinterpret_cast<const float4*>(prod + cur * (NACC * kSeqStride) + tid * kSeqStride);
                constexpr int kChunk = 8, kChunks = kSeqRows / 4 / kChunk; // 8 x 16 bytes = 32 rows per register set, 12 sets per tile
                static_assert(kChunks % 2 == 0, "two register sets alternate");
                float4 A[kChunk], B[kChunk];
#pragma unroll
                for (int i = 0; i < kChunk; ++i) A[i] = src[i];
#pragma unroll 1
                for (int c = 0; c < kChunks; c += 2) {
                    // (one basic block: the refill of A for the next trip is unconditional -- on the last trip it re-reads the tile's first rows and is discarded)
                    const int cn = c + 2 < kChunks ? c + 2 : 0;
#pragma unroll
                    for (int i = 0; i < kChunk; ++i) B[i] = src[(c + 1) * kChunk + i];
#pragma unroll
                    for (int i = 0; i < kChunk; ++i) { acc += A[i].x; acc += A[i].y; acc += A[i].z; acc += A[i].w; }
#pragma unroll
                    for (int i = 0; i < kChunk; ++i) A[i] = src[cn * kChunk + i];
#pragma unroll
                    for (int i = 0; i < kChunk; ++i) { acc += B[i].x; acc += B[i].y; acc += B[i].z; acc += B[i].w; }
                    SEQ_INTERLEAVE();
                }
            }
        } else if (producer) {
            if (t + 2 < n_tiles) load_tile(t + 2, reg);      // in flight while the products are formed
            if (t + 1 < n_tiles) produce(cur ^ 1);           // tile t + 1 from stage[cur ^ 1]
            if (t + 2 < n_tiles) store_tile(cur, reg);       // stage[cur] held tile t: consumed by produce() one iteration ago
        }
        __syncthreads();
    }
    if (consumer && tid < NACC) out[tid] = acc;
    if (tid == 0) reinterpret_cast<unsigned*>(out)[NACC] = n_pix;
}
template <int NACC, int NF, int RPP>
__global__ __launch_bounds__(kSeqThreads) void k_seq_sums(const float* __restrict__ rows, const unsigned* __restrict__ n_pix_ptr, float* __restrict__ out) {
    seq_sums_body<NACC, NF, RPP>(rows, n_pix_ptr, out);
}
// Several independent problems in ONE launch, a workgroup (= one summing wave + its producers, one CU) each.  Why it exists: kernels of different streams only run side by side when
// the streams sit on different HARDWARE queues, and the runtime maps all streams of the process onto GPU_MAX_HW_QUEUES of them (default 4; tools/queue_probe.hip: K
// one-workgroup kernels on K streams take ceil(K / queues) kernel times) -- K workgroups of one launch have no such limit (ICP's reference-order replicas: op_icp_run_many).
struct SeqBatchTable { const float* rows[kSeqBatchMax]; const unsigned* n_pix[kSeqBatchMax]; float* out[kSeqBatchMax]; };
template <int NACC, int NF, int RPP>
__global__ __launch_bounds__(kSeqThreads) void k_seq_sums_many(SeqBatchTable t) {
    seq_sums_body<NACC, NF, RPP>(t.rows[blockIdx.x], t.n_pix[blockIdx.x], t.out[blockIdx.x]);
}
constexpr size_t seq_lds_bytes(int nacc, int nf, int rpp) { return sizeof(float) * (2 * (size_t)nacc * kSeqStride + 2 * (size_t)(kSeqRows / rpp) * nf); }

// the instantiations in use, by SeqLayout
struct SeqKernels { void (*one)(const float*, const unsigned*, float*); void (*many)(SeqBatchTable); size_t lds; };
template <int NACC, int NF, int RPP>
SeqKernels seq_kernels() { return {k_seq_sums<NACC, NF, RPP>, k_seq_sums_many<NACC, NF, RPP>, seq_lds_bytes(NACC, NF, RPP)}; }
const SeqKernels kSeqKernels[3] = {seq_kernels<42, 7, 1>(), seq_kernels<42, 14, 2>(), seq_kernels<2, 2, 1>()};

} // namespace

bool seq_device_ok(int device) {
    static std::mutex mu;
    static std::map<int, bool> decided; // (a failed attempt is not repeated)
    std::lock_guard<std::mutex> lk(mu);
    auto it = decided.find(device);
    if (it != decided.end()) return it->second;
    int lds_max = 0;
    bool ok = hipSetDevice(device) == hipSuccess && hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess;
    for (const SeqKernels& k : kSeqKernels)
        ok = ok && (size_t)lds_max >= k.lds && hipFuncSetAttribute(reinterpret_cast<const void*>(k.one), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) == hipSuccess &&
             hipFuncSetAttribute(reinterpret_cast<const void*>(k.many), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return decided[device] = ok;
}

hipStream_t seq_meeting_stream(int device, SeqLayout layout) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, hipStream_t> streams;
    std::lock_guard<std::mutex> lk(mu);
    auto it = streams.find({device, (int)layout});
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { s = nullptr; (void)hipGetLastError(); }
    return streams[{device, (int)layout}] = s;
}

// ---- SeqRendezvous --------------------------------------------------------------------------------------------------------------------------------------------------
void SeqRendezvous::flush_locked() { // mu_ held
    if (!pending_.empty()) {
        hipError_t e = hipSetDevice(device_);
        SeqBatchTable t{};
        const size_t n = pending_.size();
        for (size_t i = 0; i < n && e == hipSuccess; ++i) {
            e = hipStreamWaitEvent(stream_, pending_[i]->ready, 0);
            t.rows[i] = pending_[i]->rows; t.n_pix[i] = pending_[i]->n_pix; t.out[i] = pending_[i]->out;
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kSeqKernels[layout_].many, dim3((unsigned)n), dim3(kSeqThreads), kSeqKernels[layout_].lds, stream_, t);
            e = hipGetLastError();
        }
        for (size_t i = 0; i < n && e == hipSuccess; ++i) e = hipMemcpyAsync(pending_[i]->host_out, pending_[i]->out, (seq_nacc(layout_) + 1) * sizeof(float), hipMemcpyDeviceToHost, stream_);
        const hipError_t es = hipStreamSynchronize(stream_); // (also after a failure: nothing enqueued may outlive the callers' buffers)
        if (e == hipSuccess) e = es;
        for (size_t i = 0; i < n; ++i) pending_[i]->status = e; // every request of the launch learns how it went
        pending_.clear();
    }
    arrived_ = 0;
    ++generation_;
    cv_.notify_all();
}
SeqRendezvous::Membership SeqRendezvous::join() {
    std::lock_guard<std::mutex> lk(mu_);
    ++participants_;
    return Membership(this);
}
void SeqRendezvous::pass() {
    std::lock_guard<std::mutex> lk(mu_);
    if (++arrived_ >= participants_) flush_locked();
}
void SeqRendezvous::leave() {
    std::lock_guard<std::mutex> lk(mu_);
    --participants_;
    if (participants_ > 0 && arrived_ >= participants_) flush_locked();
    if (participants_ <= 0) { participants_ = 0; arrived_ = 0; }
}
hipError_t SeqRendezvous::submit(const float* rows, const unsigned* n_pix, float* out, float* host_out, hipEvent_t ev, hipStream_t stream_of_rows) {
    SeqRequest req{rows, n_pix, out, host_out, ev, hipSuccess};
    std::unique_lock<std::mutex> lk(mu_);
    if (participants_ < minp_) { // too few to be worth meeting: counts as "nothing from me this round" for whoever does wait
        if (++arrived_ >= participants_) flush_locked();
        return hipErrorNotReady;
    }
    const hipError_t er = hipEventRecord(ev, stream_of_rows);
    if (er != hipSuccess) { if (++arrived_ >= participants_) flush_locked(); return er; }
    pending_.push_back(&req);
    if (++arrived_ >= participants_ || pending_.size() >= (size_t)kSeqBatchMax) flush_locked();
    else {
        const unsigned long long g = generation_;
        while (generation_ == g)
            if (cv_.wait_for(lk, std::chrono::milliseconds(5)) == std::cv_status::timeout && generation_ == g) flush_locked(); // (safety valve)
    }
    return req.status;
}

// ---- SeqSums ----------------------------------------------------------------------------------------------------------------------------------------------------------
hipError_t SeqSums::reserve(int device, bool from_cache) {
    if (status_ != hipErrorNotReady) return status_;
    if (!seq_device_ok(device)) return status_ = hipErrorNotSupported;
    from_cache_ = from_cache;
    auto get = [&](void** p, size_t bytes, bool pinned) {
        return from_cache ? op::cache_alloc(p, bytes, pinned) : pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    };
    hipError_t e = get((void**)&out, 64 * sizeof(float), false);
    if (e == hipSuccess) e = get((void**)&total, sizeof(unsigned), false);
    if (e == hipSuccess) e = get((void**)&host, 64 * sizeof(float), true);
    if (e == hipSuccess) e = op::cached_event(&ev);
    return status_ = e;
}
void SeqSums::release(int device) {
    op::release_event(ev, device);
    if (from_cache_) { op::cached_free(out); op::cached_free(total); op::cached_free(host); }
    else { (void)hipFree(out); (void)hipFree(total); if (host) (void)hipHostFree(host); }
    *this = SeqSums();
}
hipError_t SeqSums::run(SeqLayout layout, const float* rows, const unsigned* n_rows_host, hipStream_t stream, SeqRendezvous* meeting) {
    hipError_t e = n_rows_host ? hipMemcpyAsync(total, n_rows_host, sizeof(unsigned), hipMemcpyHostToDevice, stream) : hipSuccess; // (pageable source: staged before the call returns)
    if (e != hipSuccess) return e;
    e = meeting ? meeting->submit(rows, total, out, host, ev, stream) : hipErrorNotReady; // with the others: one launch, a workgroup each
    if (e != hipErrorNotReady) return e;
    hipLaunchKernelGGL(kSeqKernels[layout].one, dim3(1), dim3(kSeqThreads), kSeqKernels[layout].lds, stream, rows, (const unsigned*)total, out); // alone
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, out, (seq_nacc(layout) + 1) * sizeof(float), hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}

// ---- test hooks: the kernel on rows the caller makes up (see op_debug_seq_sums) -------------------------------------------------------------------------------------
namespace {
constexpr unsigned kSeqDebugMaxItems = 1u << 24;
constexpr size_t seq_item_floats(int layout) { return layout == kSeqOneRow ? 7 : layout == kSeqTwoRows ? 14 : 2; }
} // namespace

extern "C" {

int op_debug_seq_tile_rows(void) { return kSeqRows; }

int op_debug_seq_sums(int layout, const float* rows, unsigned n_uploaded, unsigned n_items, float* out) {
    if (layout < kSeqOneRow || layout > kSeqTwoValues) return op::fail(OP_ERR_INVALID, "op_debug_seq_sums: layout must be 0, 1 or 2");
    if (!out || (!rows && n_uploaded)) return op::fail(OP_ERR_INVALID, "null argument");
    if (n_items > n_uploaded || n_uploaded > kSeqDebugMaxItems) return op::fail(OP_ERR_INVALID, "op_debug_seq_sums: n_items <= n_uploaded <= 2^24");
    op::Scope scope;
    OP_TRY(scope.open(0));
    if (!seq_device_ok(0)) return op::fail(OP_ERR_NO_DEVICE, "op_debug_seq_sums: the device cannot run k_seq_sums (dynamic LDS)");
    const SeqLayout l = (SeqLayout)layout;
    const size_t floats = (size_t)n_uploaded * seq_item_floats(layout);
    float* d = nullptr;      // all n_uploaded items; stays null without any: the kernel may not touch the rows of an empty problem
    if (floats) {
        OP_TRY(scope.alloc(&d, floats));
        OP_HIP(hipMemcpy(d, rows, floats * sizeof(float), hipMemcpyHostToDevice));
    }
    SeqSums sums; // (its own hipMalloc'ed buffers: released below whatever happened)
    hipError_t e = sums.reserve(0, false);
    if (e == hipSuccess) e = sums.run(l, d, &n_items, scope.stream, nullptr);
    if (e == hipSuccess) std::memcpy(out, sums.host, (seq_nacc(l) + 1) * sizeof(float));
    (void)hipStreamSynchronize(scope.stream);
    sums.release(0);
    if (e != hipSuccess) return op::fail(OP_ERR_HIP, "op_debug_seq_sums: the sums failed: %s", hipGetErrorString(e));
    return OP_OK;
}

int op_debug_seq_sums_many(int layout, const float* const* rows, const unsigned* n_items, int k, float* out) {
    if (layout < kSeqOneRow || layout > kSeqTwoValues) return op::fail(OP_ERR_INVALID, "op_debug_seq_sums_many: layout must be 0, 1 or 2");
    if (k < 1 || k > kSeqBatchMax) return op::fail(OP_ERR_INVALID, "op_debug_seq_sums_many: 1 <= k <= %d", kSeqBatchMax);
    if (!rows || !n_items || !out) return op::fail(OP_ERR_INVALID, "null argument");
    const size_t nf = seq_item_floats(layout), words = (size_t)seq_nacc((SeqLayout)layout) + 1;
    size_t start[kSeqBatchMax], total = 0; // every problem's rows begin on a 256-byte boundary of one buffer
    for (int i = 0; i < k; ++i) {
        if (n_items[i] > kSeqDebugMaxItems || (!rows[i] && n_items[i])) return op::fail(OP_ERR_INVALID, "op_debug_seq_sums_many: problem %d: null rows or more than 2^24 items", i);
        start[i] = total;
        total += ((size_t)n_items[i] * nf + 63) / 64 * 64;
    }
    op::Scope scope;
    OP_TRY(scope.open(0));
    if (!seq_device_ok(0)) return op::fail(OP_ERR_NO_DEVICE, "op_debug_seq_sums_many: the device cannot run k_seq_sums_many (dynamic LDS)");
    float* d_rows = nullptr;
    float* d_out = nullptr;  // k x 64 words
    unsigned* d_n = nullptr;
    if (total) OP_TRY(scope.alloc(&d_rows, total));
    OP_TRY(scope.alloc(&d_out, (size_t)k * 64));
    OP_TRY(scope.alloc(&d_n, (size_t)k));
    OP_HIP(hipMemcpy(d_n, n_items, (size_t)k * sizeof(unsigned), hipMemcpyHostToDevice));
    SeqBatchTable t{};
    for (int i = 0; i < k; ++i) {
        if (n_items[i]) OP_HIP(hipMemcpy(d_rows + start[i], rows[i], (size_t)n_items[i] * nf * sizeof(float), hipMemcpyHostToDevice));
        t.rows[i] = n_items[i] ? d_rows + start[i] : nullptr; t.n_pix[i] = d_n + i; t.out[i] = d_out + (size_t)i * 64;
    }
    hipLaunchKernelGGL(kSeqKernels[layout].many, dim3((unsigned)k), dim3(kSeqThreads), kSeqKernels[layout].lds, scope.stream, t); // as SeqRendezvous::flush_locked does
    OP_HIP(hipGetLastError());
    for (int i = 0; i < k; ++i) OP_HIP(hipMemcpyAsync(out + (size_t)i * words, d_out + (size_t)i * 64, words * sizeof(float), hipMemcpyDeviceToHost, scope.stream));
    OP_HIP(hipStreamSynchronize(scope.stream));
    return OP_OK;
}

} // extern "C"
