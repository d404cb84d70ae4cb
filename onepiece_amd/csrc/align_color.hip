// align_color.hip -- tool::AlignColorToDepth (Tool/IO.cpp:9-58) on the device: the colour image of a second camera re-sampled onto the depth
// pixels, alone (op_align_color_to_depth) and as the front of the fusion path (op_volume_integrate_unaligned[_sequence]: the aligned image is
// made on the volume's stream into a ring the volume owns, and the frame then joins the queue op_volume_integrate fills as an ordinary
// device-resident frame -- k_prepare_frames, k_select* and k_integrate are untouched).
//
// The definition (restated in tests/align_color_common.py), per depth pixel (v, u) with z = depth(v, u):
//   !(z > 0)                              -> (0, 0, 0)                                              IO.cpp:46, Geometry.cpp:92,100
//   x = ((float)u - cx_d) * z / fx_d,  y = ((float)v - cy_d) * z / fy_d                              Geometry.cpp:94-96
//   q = M (x, y, z, 1) summed left to right,  p = q.xyz / q.w                                       Geometry.cpp:29-34 (as select.hip's TransformPoints)
//   a = p0 / p2, b = p1 / p2, c = p2 / p2;  uf = fx_c * a + cx_c * c,  vf = fy_c * b + cy_c * c      IO.cpp:49
//   cu = (int)((double)uf + 0.5),  cv = (int)((double)vf + 0.5)   (truncation toward zero)          IO.cpp:50-51
//   accepted when 0 <= cu < color_cam.width and 0 <= cv < DEPTH_cam.height                           IO.cpp:30-33,52 (the reference's own bound)
// Only z > 0 of the depth-camera point is tested: a point behind the colour camera is projected and sampled like any other.
// Two things the reference leaves undefined are defined as "rejected": a sum that is NaN or whose truncation does not fit an int (x86 yields
// INT_MIN there, which fails the bound; here it is tested explicitly, not left to the conversion instruction's saturation), and a (cv, cu)
// outside the colour image that was actually passed (the reference reads past its image when depth_cam.height > colour rows).
// Compiled with -ffp-contract=off like every unit: each product and sum above rounds on its own.
#include "volume_core.hpp"

namespace {

using op::check_mem;
using op::Scope;

struct AlignParams {
    float fx_d, fy_d, cx_d, cy_d, depth_scale;
    float fx_c, fy_c, cx_c, cy_c;
    int w_d, h_d;       // depth image = output size
    int u_lim, v_lim;   // accepted: 0 <= cu < u_lim, 0 <= cv < v_lim  (min of the reference's bound and the colour image's own size)
    int color_cols;     // row pitch of the colour image in pixels
    int depth_u16;
    float M[16];        // color_to_depth, row-major
};

constexpr int kTileW = 64, kTileH = 4; // one wave per image-row segment: its 64 three-byte pixels are 192 contiguous output bytes

// One thread per depth pixel; every thread writes its own three bytes (zeros when nothing is sampled), so the output needs no clearing and no
// two threads share a byte whatever the width is.
__global__ __launch_bounds__(kTileW* kTileH) void k_align_color(AlignParams A, const void* __restrict__ depth, const unsigned char* __restrict__ color,
                                                                 unsigned char* __restrict__ out) {
    const int u = blockIdx.x * kTileW + threadIdx.x, v = blockIdx.y * kTileH + threadIdx.y;
    if (u >= A.w_d || v >= A.h_d) return;
    const size_t pix = (size_t)v * A.w_d + u;
    const float z = A.depth_u16 ? (float)((const unsigned short*)depth)[pix] / A.depth_scale : ((const float*)depth)[pix];
    unsigned char c0 = 0, c1 = 0, c2 = 0;
    if (z > 0) {
        const float x = ((float)u - A.cx_d) * z / A.fx_d;
        const float y = ((float)v - A.cy_d) * z / A.fy_d;
        const float* M = A.M;
        const float q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * 1.0f;
        const float q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * 1.0f;
        const float q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * 1.0f;
        const float q3 = ((M[12] * x + M[13] * y) + M[14] * z) + M[15] * 1.0f;
        float p0 = q0, p1 = q1, p2 = q2; // x / 1 == x: the three divisions only run when some lane's w is not exactly 1 (select.hip does the same)
        if (__builtin_amdgcn_ballot_w64(q3 != 1.0f) != 0ull) { p0 = q0 / q3; p1 = q1 / q3; p2 = q2 / q3; }
        const float a = p0 / p2, b = p1 / p2, c = p2 / p2;
        const float uf = A.fx_c * a + A.cx_c * c;
        const float vf = A.fy_c * b + A.cy_c * c;
        const double du = (double)uf + 0.5, dv = (double)vf + 0.5;
        // NaN fails every comparison; the open interval is exactly the doubles whose truncation is an int
        if (du > -2147483649.0 && du < 2147483648.0 && dv > -2147483649.0 && dv < 2147483648.0) {
            const int cu = (int)du, cv = (int)dv;
            if (cu >= 0 && cu < A.u_lim && cv >= 0 && cv < A.v_lim) {
                const unsigned char* s = color + 3 * ((size_t)cv * A.color_cols + cu);
                c0 = s[0]; c1 = s[1]; c2 = s[2];
            }
        }
    }
    unsigned char* o = out + 3 * pix;
    o[0] = c0; o[1] = c1; o[2] = c2;
}

int check_align_args(const op_camera* color_cam, const op_camera* depth_cam, int color_rows, int color_cols, int depth_fmt) {
    if (!color_cam || !depth_cam) return fail(OP_ERR_INVALID, "null camera");
    if (depth_cam->width <= 0 || depth_cam->height <= 0 || color_cam->width <= 0 || color_cam->height <= 0 || color_rows <= 0 || color_cols <= 0)
        return fail(OP_ERR_INVALID, "image and camera sizes must be positive");
    if ((long long)depth_cam->width * depth_cam->height > 0x7fffffffLL / 4 || (long long)color_rows * color_cols > 0x7fffffffLL / 3)
        return fail(OP_ERR_INVALID, "image too large");
    if (depth_fmt != OP_DEPTH_F32 && depth_fmt != OP_DEPTH_U16) return fail(OP_ERR_INVALID, "unknown depth format %d", depth_fmt);
    return OP_OK;
}

// enqueues the kernel; d_depth (depth camera's size), d_color (color_rows x color_cols x 3) and d_out are device memory
void launch_align(hipStream_t stream, const op_camera& cc, const op_camera& dc, const unsigned char* d_color, int color_rows, int color_cols, const void* d_depth,
                  int depth_fmt, const float* color_to_depth, unsigned char* d_out) {
    AlignParams A;
    A.fx_d = dc.fx; A.fy_d = dc.fy; A.cx_d = dc.cx; A.cy_d = dc.cy; A.depth_scale = dc.depth_scale;
    A.fx_c = cc.fx; A.fy_c = cc.fy; A.cx_c = cc.cx; A.cy_c = cc.cy;
    A.w_d = dc.width; A.h_d = dc.height;
    A.u_lim = std::min(cc.width, color_cols);  // IO.cpp:32, and never past the row that was passed
    A.v_lim = std::min(dc.height, color_rows); // IO.cpp:33 (the DEPTH camera's height), and never past the image that was passed
    A.color_cols = color_cols;
    A.depth_u16 = depth_fmt == OP_DEPTH_U16;
    static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(A.M, color_to_depth ? color_to_depth : kIdentity, sizeof(A.M));
    const dim3 grid((unsigned)((dc.width + kTileW - 1) / kTileW), (unsigned)((dc.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(k_align_color, grid, dim3(kTileW, kTileH), 0, stream, A, d_depth, d_color, d_out);
}

// ---- the volume's ring of aligned images -------------------------------------------------------------------------------------------------
// A queued frame keeps pointing at its aligned image (and, for a host frame, at the device copy of its depth image) until its batch is launched,
// and a launched batch until it is CONFIRMED complete: a replay after pool growth reads the images again (op_volume::log).  Frames are accepted,
// launched and retired in order, so slot s -- last given to the frame with ordinal ua_frame[s] -- is free exactly when that ordinal is not above
// the number of frames done.  kUaSlots = 2 x kMaxBatch: the queue holds fewer than kMaxBatch frames, so the slot about to be reused belongs to a
// batch launched at least kMaxBatch frames ago, which has normally been confirmed by then; if not, the call waits for it (vol_check).

uint64_t frames_done(op_volume* v) {
    vol_retire(v);
    uint64_t open = (uint64_t)v->pend_n;
    for (const auto& r : v->log) open += (uint64_t)r.nf;
    return v->frames_accepted >= open ? v->frames_accepted - open : 0;
}

size_t ua_rgb_pitch(size_t npx) { return (npx * 3 + 255) & ~(size_t)255; } // keeps every slot 4-byte aligned for k_prepare_frames' wide colour loads

int ua_ensure(op_volume* v, bool host_depth) {
    const size_t npx = (size_t)v->cam.width * v->cam.height;
    if (v->ua_px != npx) {
        if (v->ua_rgb || v->ua_depth) OP_TRY(vol_check(v)); // nothing queued or replayable may still point into the old ring
        if (v->ua_rgb) op::cached_free(v->ua_rgb);
        if (v->ua_depth) op::cached_free(v->ua_depth);
        v->ua_rgb = nullptr; v->ua_depth = nullptr; v->ua_px = 0;
        for (auto& f : v->ua_frame) f = 0;
        OP_HIP(op::cached_malloc((void**)&v->ua_rgb, (size_t)op_volume::kUaSlots * ua_rgb_pitch(npx)));
        v->ua_px = npx;
    }
    if (host_depth && !v->ua_depth) OP_HIP(op::cached_malloc((void**)&v->ua_depth, (size_t)op_volume::kUaSlots * npx * 4));
    return OP_OK;
}

int ua_acquire(op_volume* v, int* slot) {
    const int s = (int)(v->ua_next++ % (unsigned)op_volume::kUaSlots);
    if (v->ua_frame[s] > frames_done(v)) OP_TRY(vol_check(v)); // launches what is queued, waits, retires everything
    *slot = s;
    return OP_OK;
}

// device copy of a host colour image, for the kernel only: two buffers taken in turn, each free again when the kernel that read it has run
int ua_stage_color(op_volume* v, const unsigned char* color, size_t bytes, unsigned char** d_color, int* which) {
    const int k = (int)(v->ua_color_next++ & 1u);
    if (v->ua_color_used[k]) OP_HIP(hipEventSynchronize(v->ua_color_done[k]));
    v->ua_color_used[k] = false;
    if (v->ua_color_cap[k] < bytes) {
        if (v->ua_color[k]) op::cached_free(v->ua_color[k]);
        v->ua_color[k] = nullptr; v->ua_color_cap[k] = 0;
        OP_HIP(op::cached_malloc((void**)&v->ua_color[k], bytes));
        v->ua_color_cap[k] = bytes;
    }
    if (!v->ua_color_done[k]) OP_HIP(op::cached_event(&v->ua_color_done[k]));
    const void* part = color;
    const size_t zero = 0;
    OP_TRY(write_staged(v->ua_color[k], 1, &part, &bytes, &zero, v->device)); // complete on return: the caller's image is free again
    *d_color = v->ua_color[k];
    *which = k;
    return OP_OK;
}

int integrate_unaligned(op_volume* v, const void* depth, int depth_fmt, const unsigned char* color, int color_rows, int color_cols, const op_camera* color_cam,
                        const float* color_to_depth, int mem, const float pose[16], const float* pose_inv) {
    if (v->pend_n > 0 && v->pend_fmt != depth_fmt) OP_TRY(vol_flush(v));
    OP_TRY(ua_ensure(v, mem == OP_MEM_HOST));
    int s = 0;
    OP_TRY(ua_acquire(v, &s));
    const size_t npx = v->ua_px;
    unsigned char* aligned = v->ua_rgb + (size_t)s * ua_rgb_pitch(npx);
    const unsigned char* d_color = color;
    int staged = -1;
    if (mem == OP_MEM_HOST) {
        void* d_depth = v->ua_depth + (size_t)s * npx * 4;
        const size_t dbytes = npx * (depth_fmt == OP_DEPTH_U16 ? 2 : 4), zero = 0;
        OP_TRY(write_staged(d_depth, 1, &depth, &dbytes, &zero, v->device));
        depth = d_depth;
        unsigned char* dc = nullptr;
        OP_TRY(ua_stage_color(v, color, (size_t)color_rows * color_cols * 3, &dc, &staged));
        d_color = dc;
    }
    launch_align(v->stream, *color_cam, v->cam, d_color, color_rows, color_cols, depth, depth_fmt, color_to_depth, aligned);
    OP_HIP(hipGetLastError());
    if (staged >= 0) {
        OP_HIP(hipEventRecord(v->ua_color_done[staged], v->stream));
        v->ua_color_used[staged] = true;
    }
    // from here on the frame is what op_volume_integrate queues for OP_MEM_DEVICE images
    const int slot = v->pend_n;
    frame_params(v, pose, pose_inv, &v->pend_F.f[slot], &v->pend_I.f[slot]);
    v->pend_P.depth[slot] = depth;
    v->pend_P.rgb[slot] = aligned;
    v->pend_fmt = depth_fmt;
    v->ua_frame[s] = ++v->frames_accepted;
    if (++v->pend_n == kMaxBatch) return vol_flush(v);
    return OP_OK;
}

} // namespace

namespace opv {
void vol_release_aligned(op_volume* v) { // op_volume_destroy: both streams have been synchronised
    if (v->ua_rgb) op::cached_free(v->ua_rgb);
    if (v->ua_depth) op::cached_free(v->ua_depth);
    for (int k = 0; k < 2; ++k) {
        if (v->ua_color[k]) op::cached_free(v->ua_color[k]);
        op::release_event(v->ua_color_done[k], v->device);
    }
}
} // namespace opv

extern "C" {

int op_align_color_to_depth(const op_camera* color_cam, const op_camera* depth_cam, const uint8_t* color, int color_rows, int color_cols, const void* depth,
                            int depth_fmt, const float* color_to_depth, int mem, int device, uint8_t* aligned_out) {
    if (!color || !depth || !aligned_out) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_align_args(color_cam, depth_cam, color_rows, color_cols, depth_fmt));
    OP_TRY(check_mem(mem));
    const size_t npx = (size_t)depth_cam->width * depth_cam->height;
    Scope s;
    OP_TRY(s.open(device));
    const unsigned char *d_depth = nullptr, *d_color = nullptr;
    OP_TRY(s.input(static_cast<const unsigned char*>(depth), npx * (depth_fmt == OP_DEPTH_U16 ? 2 : 4), mem, &d_depth));
    OP_TRY(s.input(color, (size_t)color_rows * color_cols * 3, mem, &d_color));
    unsigned char* d_out = aligned_out;
    if (mem == OP_MEM_HOST) OP_TRY(s.alloc(&d_out, npx * 3));
    launch_align(s.stream, *color_cam, *depth_cam, d_color, color_rows, color_cols, d_depth, depth_fmt, color_to_depth, d_out);
    OP_HIP(hipGetLastError());
    if (mem == OP_MEM_HOST) return s.output(aligned_out, static_cast<const unsigned char*>(d_out), npx * 3, mem);
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

int op_volume_integrate_unaligned(op_volume* v, const void* depth, int depth_fmt, const uint8_t* color, int color_rows, int color_cols, const op_camera* color_cam,
                                  const float* color_to_depth, int mem, const float pose[16], const float* pose_inv) {
    OP_VOL(v);
    if (!depth || !color || !pose) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_align_args(color_cam, &v->cam, color_rows, color_cols, depth_fmt));
    OP_TRY(check_mem(mem));
    return integrate_unaligned(v, depth, depth_fmt, color, color_rows, color_cols, color_cam, color_to_depth, mem, pose, pose_inv);
}

int op_volume_integrate_unaligned_sequence(op_volume* v, const void* depth, size_t depth_stride_bytes, int depth_fmt, const uint8_t* color, size_t color_stride_bytes,
                                           int color_rows, int color_cols, const op_camera* color_cam, const float* color_to_depth, const float* poses,
                                           size_t n_frames) {
    OP_VOL(v);
    if (!depth || !color || !poses) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_align_args(color_cam, &v->cam, color_rows, color_cols, depth_fmt));
    for (size_t f = 0; f < n_frames; ++f) // the single call, frame by frame: the frames join the same queue and the same ring
        OP_TRY(integrate_unaligned(v, (const char*)depth + f * depth_stride_bytes, depth_fmt, color + f * color_stride_bytes, color_rows, color_cols, color_cam,
                                   color_to_depth, OP_MEM_DEVICE, poses + 16 * f, nullptr));
    return OP_OK;
}

} // extern "C"
