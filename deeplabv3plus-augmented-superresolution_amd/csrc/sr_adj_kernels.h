// A section of sr.hip, included inside its anonymous namespace after sr_rw_kernels.h (it uses sr_map_affine, sr_gather_copies,
// sr_prior_and_update, sr_pd_update, SrMonArg and SR_NO_PK_F32 of that file): the backward gather with the EXACT transpose of the
// forward rotate (include/asr_hip.h, "exact adjoint": the rule).  sr.hip keeps the entry points and the solve loop;
// tests/test_gpu_sr_adj.py pins these kernels against tests/sr_adj_ref.py.
#pragma once

// ---- exact adjoint ---------------------------------------------------------------------------------------------------------------
// The registered gather takes ONE bilinear tap of G_R[n] at R^-1 p.  The transpose of the forward rotate is instead the sum over
// the rotated-grid positions q whose own forward taps touch p, each with the weight the forward kernel gave x[p] when it sampled
// at q.  The weight depends on (q, p) alone and is recomputed with the forward's statements (sr_map_affine, floorf, the two
// differences); the window only has to CONTAIN every q with a non-zero weight: a q too many adds (+-0) * G.
constexpr float kAdjMargin = 1.0f / 64.0f;     // widens the half-width: the inverse is a rounded one, R^-1 p is float32
constexpr float kAdjFixedHalf = 1.46875f;      // half-width (margin included) up to which ceil(q - e) + {0, 1, 2} covers [q - e, q + e]
constexpr float kAdjMaxHalf = 8.0f;            // largest half-width the counted loop serves (17 x 17 positions); beyond: registered
constexpr float kAdjMaxShift = 16384.0f;       // |translation of the inverse| up to which float32 keeps R^-1 p within the margin
constexpr int kAdjAffineInv = 1, kAdjExact = 2, kAdjFixed3 = 4;   // the mode word of an image; bit 0 is sr_affine_flags_kernel's flag

__device__ __forceinline__ float sr_adj_half(float a, float b) { return (fabsf(a) + fabsf(b)) + kAdjMargin; }

// mode[b]: kAdjAffineInv when every inverse rotation of image b is affine (what sr_affine_flags_kernel writes), + kAdjExact when the
// exact form applies to the image, + kAdjFixed3 when, besides, every copy's window fits 3 x 3.  flags[b] (the public answer of
// asr_sr_adjoint_flags_i32): 1 when kAdjExact is set.  Either output may be nullptr.
__global__ __launch_bounds__(64) SR_NO_PK_F32 void sr_adjoint_flags_kernel(const float* __restrict__ rot_tf,
                                                                           const float* __restrict__ trans_tf,
                                                                           const float* __restrict__ inv_rot_tf,
                                                                           int* __restrict__ flags, int* __restrict__ mode, int n) {
    const int b = blockIdx.x;
    bool aff = true, exact = true, fixed = true;
    for (int i = threadIdx.x; i < n; i += 64) {
        const float* tr = rot_tf + ((int64_t)b * n + i) * 8;
        const float* tt = trans_tf + ((int64_t)b * n + i) * 8;
        const float* ti = inv_rot_tf + ((int64_t)b * n + i) * 8;
        const bool inv_affine = ti[6] == 0.0f && ti[7] == 0.0f;
        aff = aff && inv_affine;
        const bool pure = tt[0] == 1.0f && tt[1] == 0.0f && tt[3] == 0.0f && tt[4] == 1.0f && tt[6] == 0.0f && tt[7] == 0.0f;
        const float ex = sr_adj_half(ti[0], ti[1]), ey = sr_adj_half(ti[3], ti[4]);
        // every comparison is false for a NaN: a transform that is not finite takes the registered statements
        exact = exact && inv_affine && pure && tr[6] == 0.0f && tr[7] == 0.0f && ex <= kAdjMaxHalf && ey <= kAdjMaxHalf &&
                fabsf(ti[2]) <= kAdjMaxShift && fabsf(ti[5]) <= kAdjMaxShift;
        fixed = fixed && ex <= kAdjFixedHalf && ey <= kAdjFixedHalf;
    }
    const bool all_aff = __builtin_amdgcn_ballot_w64(!aff) == 0;
    const bool all_exact = __builtin_amdgcn_ballot_w64(!exact) == 0;
    const bool all_fixed = __builtin_amdgcn_ballot_w64(!fixed) == 0;
    if (threadIdx.x == 0) {
        if (flags) flags[b] = all_exact ? 1 : 0;
        if (mode) mode[b] = (all_aff ? kAdjAffineInv : 0) | (all_exact ? kAdjExact | (all_fixed ? kAdjFixed3 : 0) : 0);
    }
}

// The forward's weight of the integer coordinate p on one axis when it samples at i: the tap at floor(i) or the one after it
__device__ __forceinline__ float sr_adj_axis_weight(float i, float p) {
    const float f = floorf(i);
    const float c = f + 1.0f;
    return (f == p) ? c - i : ((c == p) ? i - f : 0.0f);
}

// c_n(p) of one copy, the 3 x 3 form: no branch, the 6 loads of the 9 positions go out together.  plane: the copy's zero-bordered
// G_R plane.  The first position is clamped to [-2, size - 1]: a window that is moved by the clamp held no position of the image,
// and the moved one then holds only positions whose weight is none or whose G_R is the border's zero.  Rows -2 .. H + 1 and
// columns -2 .. W + 1 are all the plane is read at.
__device__ __forceinline__ float sr_adj_copy3(const AsrTf8& tr, const AsrTf8& ti, const float* __restrict__ plane, int WP, int H, int W,
                                              float fx, float fy) {
    float qx, qy;
    sr_map_affine(ti, fx, fy, qx, qy);
    const float lxf = ceilf(qx - sr_adj_half(ti.a0, ti.a1)), lyf = ceilf(qy - sr_adj_half(ti.b0, ti.b1));
    const int lx = (int)__builtin_amdgcn_fmed3f(lxf, -2.0f, (float)(W - 1)), ly = (int)__builtin_amdgcn_fmed3f(lyf, -2.0f, (float)(H - 1));
    const unsigned off = (unsigned)(__mul24(ly + kGrPadY, WP * 4) + (lx + kGrPadX) * 4);
    const char* const base = reinterpret_cast<const char*>(plane);
    float c = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const char* const row = base + (size_t)a * WP * 4;           // a scalar base per row, one lane offset for all
        const asr_f2u g01 = *reinterpret_cast<const asr_f2u*>(row + off);
        const float g2 = *reinterpret_cast<const float*>(row + off + 8);
        const float g[3] = {g01.x, g01.y, g2};
        const float qyf = (float)(ly + a);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float ix, iy;
            sr_map_affine(tr, (float)(lx + k), qyf, ix, iy);
            const float wgt = sr_adj_axis_weight(iy, fy) * sr_adj_axis_weight(ix, fx);
            c = c + wgt * g[k];
        }
    }
    return c;
}

// c_n(p) of one copy, the counted form: any half-width up to kAdjMaxHalf.  Same positions first, same order (rows, then columns).
__device__ __forceinline__ float sr_adj_copy_loop(const AsrTf8& tr, const AsrTf8& ti, const float* __restrict__ plane, int WP, int H,
                                                  int W, float fx, float fy) {
    float qx, qy;
    sr_map_affine(ti, fx, fy, qx, qy);
    const float ex = sr_adj_half(ti.a0, ti.a1), ey = sr_adj_half(ti.b0, ti.b1);
    const int lx = (int)__builtin_amdgcn_fmed3f(ceilf(qx - ex), -2.0f, (float)(W - 1));
    const int ly = (int)__builtin_amdgcn_fmed3f(ceilf(qy - ey), -2.0f, (float)(H - 1));
    const int hx = (int)__builtin_amdgcn_fmed3f(floorf(qx + ex), -3.0f, (float)(W + 1));
    const int hy = (int)__builtin_amdgcn_fmed3f(floorf(qy + ey), -3.0f, (float)(H + 1));
    float c = 0.0f;
    for (int yq = ly; yq <= hy; ++yq) {
        const float* const row = plane + (size_t)(yq + kGrPadY) * WP + kGrPadX;
        const float qyf = (float)yq;
        for (int xq = lx; xq <= hx; ++xq) {
            float ix, iy;
            sr_map_affine(tr, (float)xq, qyf, ix, iy);
            const float wgt = sr_adj_axis_weight(iy, fy) * sr_adj_axis_weight(ix, fx);
            c = c + wgt * row[xq];
        }
    }
    return c;
}

// K copies at a time, as sr_gather_chunk: the contributions are independent, only the final adds are a chain, in copy order
template <int K>
__device__ __forceinline__ float sr_adj_chunk3(float g_df, const float* __restrict__ rot_tf, const float* __restrict__ inv_rot_tf,
                                               const float* __restrict__ planes, size_t plane, int WP, int H, int W, float fx, float fy) {
    float c[K];
#pragma unroll
    for (int u = 0; u < K; ++u)
        c[u] = sr_adj_copy3(asr_load_tf(rot_tf + u * 8), asr_load_tf(inv_rot_tf + u * 8), planes + u * plane, WP, H, W, fx, fy);
#pragma unroll
    for (int u = 0; u < K; ++u) g_df += c[u];
    return g_df;
}

// sr_gather_copies with the exact transpose: the running sum of the chunks before plus this chunk's copies, in copy order.  An
// image whose mode lacks kAdjExact takes sr_gather_copies itself, the registered statements (its mode word is then 0 or 1, the
// flag that function reads).
__device__ __forceinline__ float sr_gather_copies_adj(const float* __restrict__ gr_planes, const float* __restrict__ rot_tf,
                                                      const float* __restrict__ inv_rot_tf, const float* __restrict__ acc,
                                                      const int* __restrict__ mode, const SrDims& d, int b, int X, int Y, int64_t o,
                                                      int n0, int cn) {
    const int md = mode[b];
    if (!(md & kAdjExact)) return sr_gather_copies(gr_planes, inv_rot_tf, acc, mode, d, b, X, Y, o, n0, cn);
    const int H = d.H, W = d.W, WP = W + 2 * kGrPadX;
    const size_t plane = sr_gr_plane_elems(H, W);
    const float* const planes = gr_planes + (size_t)b * cn * plane;
    const float* const tfr = rot_tf + ((int64_t)b * d.n + n0) * 8;
    const float* const tfi = inv_rot_tf + ((int64_t)b * d.n + n0) * 8;
    const float fx = (float)X, fy = (float)Y;
    float g_df = (n0 == 0) ? 0.0f : acc[o];
    int n = 0;
    if (md & kAdjFixed3) {
        for (; n + 4 <= cn; n += 4) g_df = sr_adj_chunk3<4>(g_df, tfr + n * 8, tfi + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
        for (; n < cn; ++n) g_df = sr_adj_chunk3<1>(g_df, tfr + n * 8, tfi + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
    } else {
        for (; n < cn; ++n)
            g_df += sr_adj_copy_loop(asr_load_tf(tfr + n * 8), asr_load_tf(tfi + n * 8), planes + n * plane, WP, H, W, fx, fy);
    }
    return g_df;
}

// The two gather kernels are NOT marked SR_NO_PK_F32, unlike the flags kernel above: with the attribute the inline helpers they
// share with the registered gather kernels are no longer inlined on equal terms, and all eight registered gather kernels came
// out with other machine code.  Without it every kernel of the parent keeps its instructions; the packed-f32 instructions of
// these kernels go through the unit's post-pass and the build's machine-code guard like those of the registered ones.
// sr_backward_gather_pd_kernel with the exact gather: the same frozen-image handling, chunk carry and update.
template <bool WTV, bool MON = false>
__global__ __launch_bounds__(256) void sr_backward_gather_pd_adj_kernel(
    const float* __restrict__ x, float* __restrict__ x_new, const float* __restrict__ gr_planes, const float* __restrict__ rot_tf,
    const float* __restrict__ inv_rot_tf, SrPd pd, const float* __restrict__ alphas, SrDims d, float lambda_tv, float two_lambda_l2,
    float lambda_l1, float* __restrict__ x_bordered_out, float* __restrict__ acc, int n0, int cn, const int* __restrict__ mode,
    SrTvW tw, SrMonArg<MON> mon) {
    const int X = blockIdx.x * 64 + threadIdx.x;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    const int H = d.H, W = d.W;
    if (X >= W || Y >= H) return;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if constexpr (MON) {
        if (mon.stopped[b]) {
            if (n0 + cn >= d.n) {
                x_new[o] = x[o];
                pd.py_new[o] = pd.py[o];
                pd.px_new[o] = pd.px[o];
            }
            return;
        }
    }
    const float g_df = sr_gather_copies_adj(gr_planes, rot_tf, inv_rot_tf, acc, mode, d, b, X, Y, o, n0, cn);
    if (n0 + cn < d.n) { acc[o] = g_df; return; }
    sr_pd_update<WTV>(x, x_new, pd, alphas, d, b, X, Y, g_df, lambda_tv, two_lambda_l2, lambda_l1, tw, x_bordered_out);
}

// sr_backward_gather_kernel with the exact gather.
template <bool WTV, bool MON = false>
__global__ __launch_bounds__(256) void sr_backward_gather_adj_kernel(
    const float* __restrict__ x, float* __restrict__ x_new, const float* __restrict__ gr_planes, const float* __restrict__ rot_tf,
    const float* __restrict__ inv_rot_tf, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
    const float* __restrict__ alphas, float* __restrict__ grad_out, SrDims d, float lambda_tv, float two_lambda_l2, float lambda_l1,
    SrStep st, float* __restrict__ x_bordered_out, float* __restrict__ acc, int n0, int cn, const int* __restrict__ mode, SrTvW tw,
    SrMonArg<MON> mon) {
    const int X = blockIdx.x * 64 + threadIdx.x;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    const int H = d.H, W = d.W;
    if (X >= W || Y >= H) return;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if constexpr (MON) {
        if (mon.stopped[b]) {
            if (n0 + cn >= d.n) x_new[o] = x[o];
            return;
        }
    }
    const float g_df = sr_gather_copies_adj(gr_planes, rot_tf, inv_rot_tf, acc, mode, d, b, X, Y, o, n0, cn);
    if (n0 + cn < d.n) { acc[o] = g_df; return; }
    sr_prior_and_update<WTV>(x, x_new, m, v, vhat, alphas, grad_out, d, b, X, Y, g_df, lambda_tv, two_lambda_l2, lambda_l1, st, tw,
                             x_bordered_out);
}

// The launches: one place that picks the instantiation (weighted TV, monitored)
inline int sr_adjoint_flags_launch(hipStream_t s, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf, int* flags,
                                   int* mode, int batch, int n) {
    hipLaunchKernelGGL(sr_adjoint_flags_kernel, dim3((unsigned)batch), dim3(64), 0, s, rot_tf, trans_tf, inv_rot_tf, flags, mode, n);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

template <class Mon>
int sr_gather_adj_launch(hipStream_t s, bool wtv, const dim3& grid, const float* x, float* x_new, const float* gr, const float* rot_tf,
                         const float* inv_rot_tf, float* m, float* v, float* vhat, const float* alphas, float* grad_out,
                         const SrDims& d, float lambda_tv, float two_lambda_l2, float lambda_l1, const SrStep& st, float* xb, float* acc,
                         int n0, int cn, const int* mode, const SrTvW& tw, Mon mon) {
    constexpr bool MON = std::is_same<Mon, SrMonArg<true>>::value;
    const auto k = wtv ? sr_backward_gather_adj_kernel<true, MON> : sr_backward_gather_adj_kernel<false, MON>;
    hipLaunchKernelGGL(k, grid, dim3(64, 4), 0, s, x, x_new, gr, rot_tf, inv_rot_tf, m, v, vhat, alphas, grad_out, d, lambda_tv,
                       two_lambda_l2, lambda_l1, st, xb, acc, n0, cn, mode, tw, mon);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

template <class Mon>
int sr_gather_pd_adj_launch(hipStream_t s, bool wtv, const dim3& grid, const float* x, float* x_new, const float* gr,
                            const float* rot_tf, const float* inv_rot_tf, const SrPd& pd, const float* alphas, const SrDims& d,
                            float lambda_tv, float two_lambda_l2, float lambda_l1, float* xb, float* acc, int n0, int cn,
                            const int* mode, const SrTvW& tw, Mon mon) {
    constexpr bool MON = std::is_same<Mon, SrMonArg<true>>::value;
    const auto k = wtv ? sr_backward_gather_pd_adj_kernel<true, MON> : sr_backward_gather_pd_adj_kernel<false, MON>;
    hipLaunchKernelGGL(k, grid, dim3(64, 4), 0, s, x, x_new, gr, rot_tf, inv_rot_tf, pd, alphas, d, lambda_tv, two_lambda_l2, lambda_l1,
                       xb, acc, n0, cn, mode, tw, mon);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
