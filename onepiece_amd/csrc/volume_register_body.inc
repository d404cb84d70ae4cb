// volume_register_body.inc -- the body of k_volume_register and k_volume_register_batch (volume_register.hip), included once by each: one
// workgroup's share of one cloud and its row.  The includer provides V (VolView), A (RegArgs: the cloud's points, pose and first partial row),
// K (what the instantiation reads on top), the template flags ROWS / COLOR / ROBUST / OFFSET, and two macros: REG_WG, the workgroup's index
// among the REG_N_WG workgroups of its cloud.  It runs the trips base = REG_WG 256, step = REG_N_WG 256 over A.n points and writes
// A.partial[REG_WG].  The per-point arithmetic, the reduce-scatter, the butterfly and the row store exist in this one place, so a cloud's row
// is the same bits from either kernel; it is a textual body and not a __device__ function because the single kernel's instruction stream
// changes when the same statements reach it through a call (DESIGN.md section 3.9).
    static_assert(ROBUST || !OFFSET, "the per-point target value is an option of the ROBUST instantiations");
    constexpr int kSlots = ROBUST ? kRegSlotsR : COLOR ? kRegSlotsC : kRegSlots;
    constexpr int kExt = ROBUST ? 6 : 3;
    __shared__ double s_red[kRegWg / 64][kSlots];
    double total = 0.0; // lane L: slot (L >> 1) & 31 of this wave, over its trips
    double ext[kExt] = {}; // COLOR: the wave's rc rc, s s, colored over its trips (the same in every lane); ROBUST: and r r, downweighted, color_downweighted
    BlockCache bc{INT_MIN, INT_MIN, INT_MIN, -1};
    const size_t step = (size_t)REG_N_WG * kRegWg;
    for (size_t base = (size_t)REG_WG * kRegWg; base < A.n; base += step) { // (the same trips for every lane of the workgroup)
        const size_t i = base + threadIdx.x;
        float j[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, s = 0.0f;
        float jc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rcs = 0.0f, rc = 0.0f; // COLOR: zero unless the point is coloured
        bool colored = false;
        float sraw = 0.0f, runw = 0.0f; // ROBUST: the sdf and the unweighted residual of a used point
        bool down = false, cdown = false;
        int reason = -1; // 0 used, 1 invalid, 2 no gradient, 3 too far; -1: no point
        if (i < A.n) {
            const float x = A.xyz[3 * i], y = A.xyz[3 * i + 1], z = A.xyz[3 * i + 2];
            const float* M = A.T; // TransformPoints' order (k_prepare_frames)
            const float q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * 1.0f;
            const float q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * 1.0f;
            const float q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * 1.0f;
            const float q3 = ((M[12] * x + M[13] * y) + M[14] * z) + M[15] * 1.0f;
            const float p0 = q0 / q3, p1 = q1 / q3, p2 = q2 / q3;
            float sv = 0.0f, mv = 0.0f;
            reason = 1;
            float off = 0.0f; // OFFSET: the point's target value; a non-finite one leaves the point invalid (false for NaN)
            bool have = true;
            if constexpr (OFFSET) { off = K.offset[i]; have = fabsf(off) < INFINITY; }
            if (have && reg_sample_sdf<COLOR>(V, A.W, bc, p0, p1, p2, &sv, &mv)) {
                const float h = 0.5f * A.W.res; // k_rc_shade's central difference
                float d[3], g[3] = {0.0f, 0.0f, 0.0f};
                bool all = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float sp = 0.0f, sm = 0.0f, ip = 0.0f, im = 0.0f;
                    all = all && reg_sample_sdf<COLOR>(V, A.W, bc, p0 + (a == 0 ? h : 0.0f), p1 + (a == 1 ? h : 0.0f), p2 + (a == 2 ? h : 0.0f), &sp, &ip)
                              && reg_sample_sdf<COLOR>(V, A.W, bc, p0 - (a == 0 ? h : 0.0f), p1 - (a == 1 ? h : 0.0f), p2 - (a == 2 ? h : 0.0f), &sm, &im);
                    d[a] = sp - sm;
                    if constexpr (COLOR) g[a] = (ip - im) / A.W.res;
                }
                const float l2 = all ? d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]) : 0.0f;
                if (!(l2 > 0.0f)) reason = 2;
                else if (A.max_distance > 0.0f && !(fabsf(sv) <= A.max_distance)) reason = 3;
                else {
                    reason = 0;
                    const float l = sqrtf(l2);
                    float n0 = d[0] / l, n1 = d[1] / l, n2 = d[2] / l;
                    float e = sv; // what the linearisation starts from (the gate above and sraw below keep the stored sdf)
                    if constexpr (OFFSET) e = sv - off;
                    s = e;
                    if constexpr (ROBUST) { // the row vector a (in n's place) and the residual r (in s's)
                        if (K.linearization == OP_REGISTER_LIN_GRADIENT) { n0 = d[0] / A.W.res; n1 = d[1] / A.W.res; n2 = d[2] / A.W.res; }
                        else if (K.linearization == OP_REGISTER_LIN_METRIC) s = e / (l / A.W.res);
                        sraw = sv; runw = s;
                    }
                    j[0] = n0; j[1] = n1; j[2] = n2;
                    j[3] = p1 * n2 - p2 * n1; j[4] = p2 * n0 - p0 * n2; j[5] = p0 * n1 - p1 * n0;
                    if constexpr (ROBUST) {
                        if (K.huber > 0.0f) {
                            const float w = fabsf(s) <= K.huber ? 1.0f : K.huber / fabsf(s);
                            const float q = sqrtf(w);
                            down = w < 1.0f;
#pragma unroll
                            for (int a = 0; a < 6; ++a) j[a] = q * j[a];
                            s = q * s;
                        }
                    }
                    if constexpr (COLOR) {
                        const float y = K.intensity[i], r = mv - y;
                        if (fabsf(y) < INFINITY && (!(K.max_color_residual > 0.0f) || fabsf(r) <= K.max_color_residual)) { // (false for a NaN y)
                            colored = true;
                            const float cs = K.color_scale;
                            jc[0] = cs * g[0]; jc[1] = cs * g[1]; jc[2] = cs * g[2];
                            jc[3] = cs * (p1 * g[2] - p2 * g[1]); jc[4] = cs * (p2 * g[0] - p0 * g[2]); jc[5] = cs * (p0 * g[1] - p1 * g[0]);
                            rc = r; rcs = cs * r;
                            if constexpr (ROBUST) {
                                if (K.huber_color > 0.0f) {
                                    const float wc = fabsf(r) <= K.huber_color ? 1.0f : K.huber_color / fabsf(r);
                                    const float qc = sqrtf(wc);
                                    cdown = wc < 1.0f;
#pragma unroll
                                    for (int a = 0; a < 6; ++a) jc[a] = qc * jc[a];
                                    rcs = qc * rcs;
                                }
                            }
                        }
                    }
                }
            }
            if (ROWS) {
                float* o = A.rows + (COLOR ? 16 : 8) * i;
#pragma unroll
                for (int a = 0; a < 6; ++a) o[a] = j[a];
                o[6] = s; o[7] = reason == 0 ? 1.0f : 0.0f;
                if constexpr (COLOR) {
#pragma unroll
                    for (int a = 0; a < 6; ++a) o[8 + a] = jc[a];
                    o[14] = rcs; o[15] = colored ? 1.0f : 0.0f;
                }
            }
        }
        // slot k of the point: float products, widened (an unused point's j and s are zero)
        auto val = [&](auto kc) -> double {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < 21) {
                constexpr int a = k < 6 ? 0 : k < 11 ? 1 : k < 15 ? 2 : k < 18 ? 3 : k < 20 ? 4 : 5;
                constexpr int first = a == 0 ? 0 : a == 1 ? 6 : a == 2 ? 11 : a == 3 ? 15 : a == 4 ? 18 : 20;
                if constexpr (COLOR) return (double)(j[a] * j[a + (k - first)]) + (double)(jc[a] * jc[a + (k - first)]);
                else return (double)(j[a] * j[a + (k - first)]);
            } else if constexpr (k < 27) {
                if constexpr (COLOR) return (double)(s * j[k - 21]) + (double)(rcs * jc[k - 21]);
                else return (double)(s * j[k - 21]);
            } else if constexpr (k == 27) {
                if constexpr (COLOR) return (double)s * (double)s + (double)rcs * (double)rcs;
                else return (double)s * (double)s;
            } else {
                return reason == k - 28 ? 1.0 : 0.0;
            }
        };
        total += op::wave_reduce_scatter32_lazy(val);
        if constexpr (ROBUST) { // the six without a slot, by the butterfly below (without COLOR three of them are zero and stay at home)
            double e[6] = {(double)rc * (double)rc, (double)sraw * (double)sraw, colored ? 1.0 : 0.0, (double)runw * (double)runw, down ? 1.0 : 0.0, cdown ? 1.0 : 0.0};
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    if (COLOR || q == 1 || q == 3 || q == 4) e[q] += __shfl_xor(e[q], m, 64);
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) ext[q] += e[q];
        } else if constexpr (COLOR) { // the three without a slot: a butterfly, lane masks 32, 16, 8, 4, 2, 1 -- a + b is b + a, so every lane holds the same total
            double e[3] = {(double)rc * (double)rc, (double)s * (double)s, colored ? 1.0 : 0.0};
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
                for (int q = 0; q < 3; ++q) e[q] += __shfl_xor(e[q], m, 64);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) ext[q] += e[q];
        }
    }
    // one row per workgroup (every lane gets here)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((lane & 1) == 0) s_red[wave][lane >> 1] = total;
    if constexpr (COLOR || ROBUST) {
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < kExt; ++q) s_red[wave][32 + q] = ext[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double t = s_red[0][threadIdx.x];
        for (int w = 1; w < kRegWg / 64; ++w) t += s_red[w][threadIdx.x];
        A.partial[(size_t)REG_WG * kSlots + threadIdx.x] = t;
    }
