// seq_sums.hpp -- sequential float32 sums on the device: the reference adds long runs of products to float32 accumulators ONE AFTER THE OTHER
// (the dense tracker's J J^T / J r over the accepted pixels, DenseOdometryFunction.cpp:297-381; point-to-plane ICP's over the inliers, ICP.cpp:121-136),
// and the rounding of those 10^5..10^6 dependent additions is part of its result -- it moves a pose by up to 2e-4 in the tracker and, where the 6x6
// system sits at JacobiSVD's rank threshold, by up to 5e-2 in ICP (DESIGN.md sections 5, 7).  A sequential float sum cannot be re-associated; what CAN
// run side by side are its accumulators.  The kernel, its launches and the host objects below live in seq_sums.hip; icp.hip and odometry.hip use them.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

// What a problem's rows look like (the kernel's template arguments <NACC, NF, RPP>, seq_sums.hip):
//   kSeqOneRow    <42, 7, 1>   one row {J[6], r} per item: ICP's inliers, the tracker's photometric / geometric term
//   kSeqTwoRows   <42, 14, 2>  two such rows per pixel: the tracker's hybrid term
//   kSeqTwoValues <2, 2, 1>    two values per item, summed as they are: NormalizeIntensity
enum SeqLayout { kSeqOneRow, kSeqTwoRows, kSeqTwoValues };
constexpr int seq_nacc(SeqLayout l) { return l == kSeqTwoValues ? 2 : 42; }

// May this device run the kernels (~150 KB of dynamic LDS: attribute query + opt-in for every layout)?  Decided once per device; false = sum on the host.
bool seq_device_ok(int device);

// ---- several host threads take their sequential sums TOGETHER ------------------------------------------------------------------------------------------------------
// Every caller has its own stream (an ICP context's, a tracker's) and a host thread that needs the sums before it can go on.  K such threads launching k_seq_sums on K
// streams scale to the number of hardware queues of the process and no further (see k_seq_sums_many; two streams on one queue take turns).  With `min_participants` or more participants they meet instead, once per iteration: a thread records "my rows are in
// place" on its stream (the request's event) and waits; the last one to arrive launches k_seq_sums_many -- a workgroup per waiting request -- on the rendezvous's own
// stream behind those events, copies the NACC + 1 numbers of every request to its pinned buffer, synchronises and releases everybody.  A participant that has nothing
// to sum in a round says so (pass), one that is done leaves; a waiter that is not released within a few milliseconds launches what is pending itself, so progress never
// depends on the count being right.  Below that many participants submit() answers hipErrorNotReady and the caller launches its own kernel as before (that many
// independent launches run side by side on their own hardware queues; meeting only costs then).  Results do not depend on who sums with whom: the kernel body and its inputs are the stand-alone launch's.
// Measured (307 200-point ICP pairs, reference-order mode, profiles/r06_icp_hw_queues.txt): with 16 hardware queues 16 independent runs reach 4.1 k iterations/s, the
// rendezvous 5.3-5.7 k (8 contexts: 3.9 k alone, 3.1-3.6 k together -- hence 9 for ICP); with 4 queues 2.0 k against 6.5 k.  For the tracker it does not pay (odometry.hip).  A variant without rounds (a free "lane" takes whatever is pending) was
// slower at every depth: the first arrival of a wave launches alone and the rest wait a whole kernel for the next lane.
// Whose rounds they are: the object belongs to whoever meets -- an op_icp_run_many call has one of its own for its contexts (two calls never share a round), trackers
// that run at the same time share one per device (odometry.hip).  It launches on `stream`, which it does not own.
constexpr int kSeqBatchMax = 32;
struct SeqRequest { const float* rows; const unsigned* n_pix; float* out; float* host_out; hipEvent_t ready; hipError_t status; };
class SeqRendezvous {
public:
    struct Leave { void operator()(SeqRendezvous* m) const { m->leave(); } };
    using Membership = std::unique_ptr<SeqRendezvous, Leave>; // leaves on every exit path of its holder
    SeqRendezvous(SeqLayout layout, int min_participants, int device, hipStream_t stream) : layout_(layout), minp_(min_participants), device_(device), stream_(stream) {}
    Membership join();
    void pass(); // this participant has nothing to sum in this round
    // hipSuccess: host_out holds the sums.  hipErrorNotReady: too few participants -- the caller launches its own kernel (the rows and n_pix are on `stream_of_rows`).
    hipError_t submit(const float* rows, const unsigned* n_pix, float* out, float* host_out, hipEvent_t ev, hipStream_t stream_of_rows);
private:
    void leave(); // this participant's loop is over
    void flush_locked();
    const SeqLayout layout_;
    const int minp_, device_;
    const hipStream_t stream_;
    std::mutex mu_;
    std::condition_variable cv_;
    int participants_ = 0, arrived_ = 0;
    unsigned long long generation_ = 0;
    std::vector<SeqRequest*> pending_;
};

// The non-blocking stream the meetings of one kind (= layout: ICP's, the trackers') launch on, created on first use and kept per device so that no call pays for a
// stream; nullptr: not to be had (not tried again).  Meetings of different kinds do not queue behind each other.
hipStream_t seq_meeting_stream(int device, SeqLayout layout);

// "The sums of these ordered rows, please": what a context (op_icp, op_tracker) owns for it -- the device result, the device row count, the pinned copy, the event
// a meeting waits on -- allocated once, from the buffer cache (common.hpp) or with plain hipMalloc / hipHostMalloc as its owner's other buffers are.
struct SeqSums {
    float* out = nullptr;        // device: the sums, then the row count
    float* host = nullptr;       // pinned copy
    unsigned* total = nullptr;   // device: the row count
    hipEvent_t ev = nullptr;     // "my ordered rows are in place" (recorded on the owner's stream for a meeting's stream to wait on)
    hipError_t reserve(int device, bool from_cache); // the first call asks seq_device_ok and allocates, every call answers how that went (no lock, nothing to look up)
    void release(int device);    // the owner has synchronised its stream
    // Leaves the seq_nacc(layout) sums in host[0 ..] and the row count behind them (count()), and returns after they have arrived.  n_rows_host: the row count to
    // upload, or nullptr when `total` already holds it on `stream`.  With a meeting the sums are taken there; if it declines (too few participants) or there is
    // none: one workgroup on `stream`, copy, synchronise.
    hipError_t run(SeqLayout layout, const float* rows, const unsigned* n_rows_host, hipStream_t stream, SeqRendezvous* meeting);
    unsigned count(SeqLayout layout) const { unsigned n; std::memcpy(&n, host + seq_nacc(layout), sizeof(n)); return n; }
private:
    hipError_t status_ = hipErrorNotReady;
    bool from_cache_ = false;
};
