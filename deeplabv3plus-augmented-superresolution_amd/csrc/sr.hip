// Iterative TV-regularised augmented super-resolution (ASR) solver and the max/mean realign
// fusions, as fused gather kernels for gfx950.
//
// Reference (paths in /root/reference):
//   superresolution_scripts/superresolution.py:44-100   loss_function
//   superresolution_scripts/superresolution.py:102-137  augmented_superresolution (the loop)
//   superresolution_scripts/superresolution.py:139-161  max_/mean_superresolution
//   superresolution_scripts/optimizer.py:37-52          Adam / AMSGrad + ExponentialDecay
//
// The TF formulation materialises ~7 tensors of [N,H,W,1] per iteration (0.7-1.4 GB of HBM
// traffic at N=100, 512x512).  Here one iteration is two launches that touch only the
// algorithmic minimum: y / residual [N,h,w] and x + Adam state [H,W]:
//   K_fwd : residual[n,i,j] = D(T_n(R_n(x)))[i,j] - y[n,i,j]   (two-stage bilinear kept exact)
//   K_bwd : g = sum_n InvRot_n(InvTrans_n(D^T(2*lambda*residual_n)))  -- TensorFlow's registered
//           gradient of ImageProjectiveTransformV3 (inverse warp of the upstream gradient,
//           NOT the scatter adjoint) -- + TV/L2/L1 prior gradients, then the Keras
//           Adam/AMSGrad update, all in one pass over the HR pixels.
#include "asr_warp_device.h"

namespace {

constexpr int kTileX = 32, kTileY = 8;  // 256 threads = 4 waves, 2 HR rows per wave

struct SrDims {
    int batch, n, H, W, h, w, f;  // f = H / h = W / w (even)
};

// ---- x0 = tf.image.resize(y[b,0], (H,W))  (superresolution.py:112-113) -------------------
__global__ __launch_bounds__(256) void sr_init_kernel(const float* __restrict__ y, float* __restrict__ x,
                                                      SrDims d, float scale_y, float scale_x) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const float* src = y + (int64_t)b * d.n * d.h * d.w;  // copy 0 of image b
    const AsrLerp ly = asr_half_pixel(Y, scale_y, d.h);
    const AsrLerp lx = asr_half_pixel(X, scale_x, d.w);
    const float tl = src[ly.lo * d.w + lx.lo], tr = src[ly.lo * d.w + lx.hi];
    const float bl = src[ly.hi * d.w + lx.lo], br = src[ly.hi * d.w + lx.hi];
    const float top = tl + (tr - tl) * lx.t;
    const float bot = bl + (br - bl) * lx.t;
    x[((int64_t)b * d.H + Y) * d.W + X] = top + (bot - top) * ly.t;
}

// ---- zero-bordered planes ---------------------------------------------------------------------------
// The solver keeps the images its bilinear gathers sample (the current x for K_fwd, the per-copy gradient planes G_R for
// the backward gather) with a zero border: row stride W + 64 (32 zero columns each side), 2 zero rows above and below.  A
// 2 x 2 tap block whose floor coordinate is clamped to [-2, W] x [-2, H] then reads zeros exactly where the unclamped
// taps fall outside the image (TF's CONSTANT-0 fill), so a sample is two unaligned 8-byte loads with no per-tap bounds
// test and no select; the weights still come from the unclamped coordinate.  Same products and sums as
// asr_tf_bilinear over a bounds-checked reader -> bit-identical.
// 32 border columns = one 128-byte line: every row's payload then starts on a line (with 4 columns -- enough for the taps --
// each 256-byte row segment a wave writes straddled three lines: K_gt + K_bwd 68 -> 62 us per iteration at N = 100).
#if defined(ASR_DIAG_KFWD_CHECK) || defined(ASR_DIAG_KFWD_NOPK)
// unpacked arithmetic written out in asm (diagnostic builds only): the compiler can neither pair nor reorder these
__device__ __forceinline__ float dg_mul(float x, float y) { float z; asm volatile("v_mul_f32 %0, %1, %2" : "=v"(z) : "v"(x), "v"(y)); return z; }
__device__ __forceinline__ float dg_add(float x, float y) { float z; asm volatile("v_add_f32 %0, %1, %2" : "=v"(z) : "v"(x), "v"(y)); return z; }
__device__ __forceinline__ float dg_sub(float x, float y) { float z; asm volatile("v_sub_f32 %0, %1, %2" : "=v"(z) : "v"(x), "v"(y)); return z; }
#endif
#ifndef ASR_DIAG_KFWD_NOPK
#define ASR_DIAG_KFWD_NOPK 0      // bits: 1 the coordinate map, 2 the bilinear sample, 4 the translate blend + D -- that stage of K_fwd in unpacked asm
#endif
constexpr int kGrPadX = 32, kGrPadY = 2;
__host__ __device__ inline size_t sr_gr_plane_elems(int H, int W) { return (size_t)(H + 2 * kGrPadY) * (size_t)(W + 2 * kGrPadX); }
typedef float asr_f2u __attribute__((ext_vector_type(2), aligned(4)));

// plane = first element of the bordered plane (its top-left border corner), WP = W + 2 * kGrPadX.  The element offset is
// non-negative, so the loads take the scalar plane base + a 32-bit lane offset.
__device__ __forceinline__ float sr_bilinear_bordered(const float* __restrict__ plane, int WP, int H, int W, float ix, float iy) {
    const float xf = floorf(ix), yf = floorf(iy);
    // min(max(asr_coord_to_int(f), -2), size) with the clamp done on the float (exact: f is an integer, the bounds are small):
    // one v_med3_f32 + one conversion per coordinate instead of four instructions; a NaN gives -2 either way (v_med3 returns
    // the minimum of the other two, asr_coord_to_int -1e9).  The gathers are bound by VALU issue.
    const int x0 = (int)__builtin_amdgcn_fmed3f(xf, -2.0f, (float)W), y0 = (int)__builtin_amdgcn_fmed3f(yf, -2.0f, (float)H);
    // byte offset in 32 bits: the loads take the scalar plane base + this lane offset (no 64-bit vector arithmetic)
    // (y0 + pad) * row bytes + (x0 + pad) * 4 as one 24-bit multiply-add (|y0|, row bytes < 2^23) and one shift-add
    const unsigned off = (unsigned)(__mul24(y0, WP * 4) + (kGrPadY * WP * 4 + kGrPadX * 4) + x0 * 4);
    const char* const base = reinterpret_cast<const char*>(plane);
    const char* const base_next = base + WP * 4;               // the next row through a second SCALAR base, not a lane add
    const asr_f2u top = *reinterpret_cast<const asr_f2u*>(base + off);
    const asr_f2u bot = *reinterpret_cast<const asr_f2u*>(base_next + off);
#ifdef ASR_DIAG_KFWD_WAIT      // diagnostic: every sample waits for its own two loads before any arithmetic on them (no loads in flight
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // of THIS wave while its packed ops execute)
#endif
#if ASR_DIAG_KFWD_NOPK & 2
    const float wxl = dg_sub(dg_add(xf, 1.0f), ix), wxh = dg_sub(ix, xf);
    const float vyf = dg_add(dg_mul(wxl, top.x), dg_mul(wxh, top.y));
    const float vyc = dg_add(dg_mul(wxl, bot.x), dg_mul(wxh, bot.y));
    return dg_add(dg_mul(dg_sub(dg_add(yf, 1.0f), iy), vyf), dg_mul(dg_sub(iy, yf), vyc));
#else
    const float wxl = (xf + 1.0f) - ix, wxh = ix - xf;
    const float vyf = wxl * top.x + wxh * top.y;
    const float vyc = wxl * bot.x + wxh * bot.y;
    return ((yf + 1.0f) - iy) * vyf + (iy - yf) * vyc;
#endif
}

// asr_tf_map for a transform known to be affine (c0 == c1 == 0): the same two expressions without the (uniform) branch
// on the projective terms -- a branch inside a sampling loop makes the compiler wait for each sample's loads in turn.
__device__ __forceinline__ void sr_map_affine(const AsrTf8& t, float x, float y, float& ix, float& iy) {
#if ASR_DIAG_KFWD_NOPK & 1
    ix = dg_add(dg_add(dg_mul(t.a0, x), dg_mul(t.a1, y)), t.a2);
    iy = dg_add(dg_add(dg_mul(t.b0, x), dg_mul(t.b1, y)), t.b2);
#else
    ix = t.a0 * x + t.a1 * y + t.a2;
    iy = t.b0 * x + t.b1 * y + t.b2;
#endif
}

#ifdef ASR_DIAG_KFWD_CHECK
// Diagnostic build only (tools/build_hazard_variants.py "kfwd_check"): K_fwd re-derives every intermediate of its fast path with
// UNPACKED arithmetic written out in asm (v_mul_f32 / v_add_f32 / v_sub_f32 never went wrong) and counts, stage by stage, where
// the compiler's (packed) code disagrees -- which of its packed-f32 sequences fails beside co-resident MFMA waves.
//   counters: 0 map ix   1 map iy   2 bilinear (weights / blend)   3 translate blend Tq   4 final D   5 waves with any mismatch
//             8 + lane (64): mismatching lanes   80 + 4 * a + c... (9): which of the 3 x 3 rotation samples (map stage)
//   records (first 16 mismatches): stage, lane, inputs, got, expected
__device__ unsigned g_kfwd_cnt[128];
__device__ float g_kfwd_rec[16][12];
__device__ __forceinline__ bool dg_ne(float a, float b) { return __float_as_int(a) != __float_as_int(b); }
__device__ __forceinline__ void dg_record(int stage, float i0, float i1, float i2, float i3, float i4, float i5, float got, float want) {
    atomicAdd(&g_kfwd_cnt[stage], 1u);
    atomicAdd(&g_kfwd_cnt[8 + ((threadIdx.y * kTileX + threadIdx.x) & 63)], 1u);
    const unsigned k = atomicAdd(&g_kfwd_cnt[7], 1u);
    if (k < 16) {
        float* r = g_kfwd_rec[k];
        r[0] = (float)stage; r[1] = (float)((threadIdx.y * kTileX + threadIdx.x) & 63);
        r[2] = i0; r[3] = i1; r[4] = i2; r[5] = i3; r[6] = i4; r[7] = i5; r[8] = got; r[9] = want;
        r[10] = (float)blockIdx.z; r[11] = (float)(blockIdx.y * 1000 + blockIdx.x);
    }
}
#endif

// ---- K_fwd --------------------------------------------------------------------------------
// One thread per LR residual element (b, n, i, j).  BORDERED: x is the solver's zero-bordered copy [batch, H+4, W+64].
#ifdef ASR_DIAG_KFWD_MAX_VGPR
#define ASR_KFWD_ATTR __attribute__((amdgpu_num_vgpr(ASR_DIAG_KFWD_MAX_VGPR)))
#else
#define ASR_KFWD_ATTR
#endif
// DT: the data term of asr_sr_data_term (include/asr_hip.h, "data term").  The DT = false instantiations take an empty
// argument and write the raw residual r, as they always did; the DT = true ones write q = w * psi(r) to `resid` -- what the
// backward kernels then read as "the residual" -- and, on request, r itself.  loss, the weights and r_out are uniform: three
// scalar branches after the gathers, one more 4-byte load per element when there are weights.
template <bool DT>
struct SrDtArg {};
template <>
struct SrDtArg<true> {
    int loss;                 // ASR_DF_*
    float delta;              // Huber's threshold
    const float* w;           // [batch, n, h, w] or [n, h, w] (stride 0), or nullptr: unweighted, no multiply at all
    int64_t w_stride;         // floats between the weights of two images: n * h * w, or 0 for one stack shared by the batch
    float* r_out;             // the raw residual as well, or nullptr
};
typedef SrDtArg<true> SrDt;

// psi = rho' / 2 of the data term, one statement per loss; a NaN residual stays a NaN under L2 and Huber
__device__ __forceinline__ float sr_dt_psi(float r, int loss, float delta) {
    if (loss == ASR_DF_L1) return (r > 0.0f) ? 0.5f : ((r < 0.0f) ? -0.5f : 0.0f);
    if (loss == ASR_DF_HUBER) return (r < -delta) ? -delta : ((r > delta) ? delta : r);
    return r;
}

// MON: the monitored solve (asr_sr_solve_mon_f32; include/asr_hip.h, "convergence monitor").  The MON = false instantiations
// take an empty argument and are the kernels they always were; in the MON = true ones the workgroups of an image whose
// stop flag is set return at once (the flag is uniform over a workgroup: one scalar load and branch).
template <bool MON>
struct SrMonArg {};
template <>
struct SrMonArg<true> {
    const int* stopped;       // [batch]: != 0 once the stop rule has frozen the image (sr_mon_decide_kernel)
};

template <bool BORDERED, bool DT = false, bool MON = false>
__global__ __launch_bounds__(256) ASR_KFWD_ATTR void sr_forward_residual_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ rot_tf,
    const float* __restrict__ trans_tf, float* __restrict__ resid, SrDims d, SrDtArg<DT> dt, SrMonArg<MON> mon) {
#ifdef ASR_DIAG_KFWD_TOP_VGPR
    ASR_DIAG_TOUCH_VGPR(ASR_DIAG_KFWD_TOP_VGPR);
#endif
    const int j = blockIdx.x * kTileX + threadIdx.x;
    const int i = blockIdx.y * kTileY + threadIdx.y;
    const int bn = blockIdx.z;  // b * n + copy
    if (j >= d.w || i >= d.h) return;
    const int b = bn / d.n;
    if constexpr (MON) {
        if (mon.stopped[b]) return;
    }
    const int H = d.H, W = d.W, WP = W + 2 * kGrPadX;
    const float* img = BORDERED ? x + (size_t)b * sr_gr_plane_elems(H, W) : x + (int64_t)b * H * W;
    const AsrTf8 tr = asr_load_tf(rot_tf + (int64_t)bn * 8);
    const AsrTf8 tt = asr_load_tf(trans_tf + (int64_t)bn * 8);

    // Branch-free taps: clamp the index, load unconditionally, select afterwards -- the 64 image taps of one
    // residual element are then issued back to back instead of one exec-masked branch + wait each.
    auto rd_x = [&](int yy, int xx) -> float {
        const bool ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W);
        const float v = img[ok ? yy * W + xx : 0];
        return ok ? v : 0.0f;
    };
    auto rd_rot = [&](int yr, int xr) -> float {
        const bool ok = (yr >= 0) & (yr < H) & (xr >= 0) & (xr < W);
        float v;
        if (BORDERED) {
            float ix, iy;
            v = asr_tf_map(tr, (float)xr, (float)yr, ix, iy) ? sr_bilinear_bordered(img, WP, H, W, ix, iy) : 0.0f;
        } else {
            v = asr_tf_sample(tr, rd_x, xr, yr);
        }
        return ok ? v : 0.0f;
    };
    auto T = [&](int yt, int xt) -> float { return asr_tf_sample(tt, rd_rot, xt, yt); };

    // D: half-pixel bilinear, even integer factor f -> taps (f*o + f/2 - 1, +1), lerp 0.5
    const int y0 = d.f * i + d.f / 2 - 1, x0 = d.f * j + d.f / 2 - 1;
    float tl, trv, bl, br;
    // Pure translation (always, for tfa.image.translate): the four T pixels read a 3 x 3 block of R pixels
    // (2 x 2 taps each, shifted by one); evaluate those 9 rotation samples once instead of 16 times.  Same
    // per-tap arithmetic as the generic path, so the results are bit-identical; the generic path stays for
    // other transforms and for the (float-rounding) case where the two tap columns / rows do not abut.
    const bool pure_translation = (tt.a0 == 1.0f) & (tt.a1 == 0.0f) & (tt.b0 == 0.0f) & (tt.b1 == 1.0f) &
                                  (tt.c0 == 0.0f) & (tt.c1 == 0.0f);
    const float jx0 = (float)x0 + tt.a2, jx1 = (float)(x0 + 1) + tt.a2;
    const float jy0 = (float)y0 + tt.b2, jy1 = (float)(y0 + 1) + tt.b2;
    const float fx0 = floorf(jx0), fx1 = floorf(jx1), fy0 = floorf(jy0), fy1 = floorf(jy1);
    const int cx0 = asr_coord_to_int(fx0), cx1 = asr_coord_to_int(fx1);
    const int cy0 = asr_coord_to_int(fy0), cy1 = asr_coord_to_int(fy1);
    const bool rot_affine = (tr.c0 == 0.0f) & (tr.c1 == 0.0f);
    if (pure_translation && cx1 == cx0 + 1 && cy1 == cy0 + 1) {
        float rv[3][3];
        if (BORDERED && rot_affine) {   // no branch inside: the 18 loads of the 9 samples go out together
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int yr = cy0 + a, xr = cx0 + c;
                    float ix, iy;
                    sr_map_affine(tr, (float)xr, (float)yr, ix, iy);
                    const float v = sr_bilinear_bordered(img, WP, H, W, ix, iy);
                    rv[a][c] = ((yr >= 0) & (yr < H) & (xr >= 0) & (xr < W)) ? v : 0.0f;
#ifdef ASR_DIAG_KFWD_CHECK
                    {
                        const float fx = (float)xr, fy = (float)yr;
                        const float ex = dg_add(dg_add(dg_mul(tr.a0, fx), dg_mul(tr.a1, fy)), tr.a2);
                        const float ey = dg_add(dg_add(dg_mul(tr.b0, fx), dg_mul(tr.b1, fy)), tr.b2);
                        if (dg_ne(ix, ex)) { dg_record(0, fx, fy, tr.a0, tr.a1, tr.a2, (float)(3 * a + c), ix, ex); atomicAdd(&g_kfwd_cnt[80 + 3 * a + c], 1u); }
                        if (dg_ne(iy, ey)) { dg_record(1, fx, fy, tr.b0, tr.b1, tr.b2, (float)(3 * a + c), iy, ey); atomicAdd(&g_kfwd_cnt[80 + 3 * a + c], 1u); }
                        // the bilinear sample from the EXPECTED coordinates, unpacked (same loads: clamped floor, two 8-byte taps)
                        const float xf = floorf(ex), yf = floorf(ey);
                        const int x0 = (int)__builtin_amdgcn_fmed3f(xf, -2.0f, (float)W), y0 = (int)__builtin_amdgcn_fmed3f(yf, -2.0f, (float)H);
                        const float* q = img + (size_t)(y0 + kGrPadY) * WP + (x0 + kGrPadX);
                        const float t0 = q[0], t1 = q[1], b0 = q[WP], b1 = q[WP + 1];
                        const float wxl = dg_sub(dg_add(xf, 1.0f), ex), wxh = dg_sub(ex, xf);
                        const float vyf = dg_add(dg_mul(wxl, t0), dg_mul(wxh, t1)), vyc = dg_add(dg_mul(wxl, b0), dg_mul(wxh, b1));
                        const float ev = dg_add(dg_mul(dg_sub(dg_add(yf, 1.0f), ey), vyf), dg_mul(dg_sub(ey, yf), vyc));
                        if (!dg_ne(ix, ex) && !dg_ne(iy, ey) && dg_ne(v, ev)) dg_record(2, ex, ey, t0, t1, b0, b1, v, ev);
                    }
#endif
                }
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) rv[a][c] = rd_rot(cy0 + a, cx0 + c);
        }
#if ASR_DIAG_KFWD_NOPK & 4
        const float wxl0 = dg_sub(dg_add(fx0, 1.0f), jx0), wxh0 = dg_sub(jx0, fx0), wxl1 = dg_sub(dg_add(fx1, 1.0f), jx1), wxh1 = dg_sub(jx1, fx1);
        const float wyl0 = dg_sub(dg_add(fy0, 1.0f), jy0), wyh0 = dg_sub(jy0, fy0), wyl1 = dg_sub(dg_add(fy1, 1.0f), jy1), wyh1 = dg_sub(jy1, fy1);
        auto Tq = [&](int a, int c, float wxl, float wxh, float wyl, float wyh) -> float {
            const float vyf = dg_add(dg_mul(wxl, rv[a][c]), dg_mul(wxh, rv[a][c + 1]));
            const float vyc = dg_add(dg_mul(wxl, rv[a + 1][c]), dg_mul(wxh, rv[a + 1][c + 1]));
            return dg_add(dg_mul(wyl, vyf), dg_mul(wyh, vyc));
        };
#else
        const float wxl0 = (fx0 + 1.0f) - jx0, wxh0 = jx0 - fx0, wxl1 = (fx1 + 1.0f) - jx1, wxh1 = jx1 - fx1;
        const float wyl0 = (fy0 + 1.0f) - jy0, wyh0 = jy0 - fy0, wyl1 = (fy1 + 1.0f) - jy1, wyh1 = jy1 - fy1;
        auto Tq = [&](int a, int c, float wxl, float wxh, float wyl, float wyh) -> float {
            const float vyf = wxl * rv[a][c] + wxh * rv[a][c + 1];
            const float vyc = wxl * rv[a + 1][c] + wxh * rv[a + 1][c + 1];
            return wyl * vyf + wyh * vyc;
        };
#endif
        tl = Tq(0, 0, wxl0, wxh0, wyl0, wyh0);
        trv = Tq(0, 1, wxl1, wxh1, wyl0, wyh0);
        bl = Tq(1, 0, wxl0, wxh0, wyl1, wyh1);
        br = Tq(1, 1, wxl1, wxh1, wyl1, wyh1);
#ifdef ASR_DIAG_KFWD_CHECK
        {
            auto eTq = [&](int a, int c, float jx, float fxx, float jy, float fyy) -> float {
                const float wl = dg_sub(dg_add(fxx, 1.0f), jx), wh = dg_sub(jx, fxx), yl = dg_sub(dg_add(fyy, 1.0f), jy), yh = dg_sub(jy, fyy);
                const float vf = dg_add(dg_mul(wl, rv[a][c]), dg_mul(wh, rv[a][c + 1]));
                const float vc = dg_add(dg_mul(wl, rv[a + 1][c]), dg_mul(wh, rv[a + 1][c + 1]));
                return dg_add(dg_mul(yl, vf), dg_mul(yh, vc));
            };
            const float e0 = eTq(0, 0, jx0, fx0, jy0, fy0), e1 = eTq(0, 1, jx1, fx1, jy0, fy0), e2 = eTq(1, 0, jx0, fx0, jy1, fy1),
                        e3 = eTq(1, 1, jx1, fx1, jy1, fy1);
            if (dg_ne(tl, e0)) dg_record(3, jx0, jy0, rv[0][0], rv[0][1], rv[1][0], rv[1][1], tl, e0);
            if (dg_ne(trv, e1)) dg_record(3, jx1, jy0, rv[0][1], rv[0][2], rv[1][1], rv[1][2], trv, e1);
            if (dg_ne(bl, e2)) dg_record(3, jx0, jy1, rv[1][0], rv[1][1], rv[2][0], rv[2][1], bl, e2);
            if (dg_ne(br, e3)) dg_record(3, jx1, jy1, rv[1][1], rv[1][2], rv[2][1], rv[2][2], br, e3);
        }
#endif
    } else {
        tl = T(y0, x0); trv = T(y0, x0 + 1);
        bl = T(y0 + 1, x0); br = T(y0 + 1, x0 + 1);
    }
    const float top = tl + (trv - tl) * 0.5f;
    const float bot = bl + (br - bl) * 0.5f;
    const float dval = top + (bot - top) * 0.5f;
    const int64_t o = ((int64_t)bn * d.h + i) * d.w + j;
    if constexpr (DT) {
        const float r = dval - y[o];
        if (dt.r_out) dt.r_out[o] = r;
        float q = sr_dt_psi(r, dt.loss, dt.delta);
        if (dt.w) q = dt.w[(int64_t)b * dt.w_stride + (o - (int64_t)b * d.n * d.h * d.w)] * q;
        resid[o] = q;
    } else {
        resid[o] = dval - y[o];
    }
#ifdef ASR_DIAG_KFWD_CHECK
    {
        const float et = dg_add(tl, dg_mul(dg_sub(trv, tl), 0.5f)), eb = dg_add(bl, dg_mul(dg_sub(br, bl), 0.5f));
        const float ed = dg_add(et, dg_mul(dg_sub(eb, et), 0.5f));
        if (dg_ne(dval, ed)) dg_record(4, tl, trv, bl, br, top, bot, dval, ed);
    }
#endif
}

// ---- K_bwd --------------------------------------------------------------------------------
// Update rule and prior of one solver step (from asr_sr_config, include/asr_hip.h).
struct SrStep {
    int optimizer, flag;      // ASR_OPT_*, amsgrad / nesterov
    float c0, c1, c2;         // hyper-parameters, meaning per optimizer (asr_hip.h)
    int prior, btv_shift;     // ASR_PRIOR_*, bilateral-TV window
    float btv_w[9];           // alpha^k, k = |h| + |v| (float32 pow like tf.pow)
};

// Edge weights of the weighted TV prior (include/asr_hip.h: the rule): wy[Y,X] prices the jump (Y,X) -> (Y+1,X), wx[Y,X] the
// jump (Y,X) -> (Y,X+1).  Read only by the WTV = true instantiations; the others never touch the argument.
struct SrTvW {
    const float* wy;
    const float* wx;
    int64_t stride;           // floats between the planes of two images: H * W, or 0 for one pair shared by the batch
};

// One axis of the inverse-translate stage for one integer G_R coordinate c (pure translation:
// the map is c + shift exactly, so x and y separate).  Bitwise the same values the generic
// asr_tf_sample path produces, computed once per axis instead of once per tap.
struct SrAxisTap {
    float wl, wh;   // (c_ceil - pos), (pos - c_floor)
    int l0, l1;     // LR index of the two G_T taps, or -1 when that tap is structurally zero
    bool inb;       // c itself inside the image (else G_R(c) = 0)
};

template <int LOG2F>
__device__ __forceinline__ int sr_gt_index(int t, int size, int f, int ph0, int ph1) {
    // G_T = ResizeBilinearGrad(g_D) is non-zero only on the 2x2 centre of every f x f block
    if (t < 0 || t >= size) return -1;
    const int ph = (LOG2F > 0) ? (t & (f - 1)) : (t % f);
    if (ph != ph0 && ph != ph1) return -1;
    return (LOG2F > 0) ? (t >> LOG2F) : (t / f);
}

template <int LOG2F>
__device__ __forceinline__ SrAxisTap sr_axis_tap(int c, float shift, int size, int f, int ph0, int ph1) {
    SrAxisTap a;
    a.inb = (c >= 0 && c < size);
    const float pos = (float)c + shift;
    const float fl = floorf(pos);
    a.wl = (fl + 1.0f) - pos;
    a.wh = pos - fl;
    const int t0 = asr_coord_to_int(fl);
    a.l0 = sr_gt_index<LOG2F>(t0, size, f, ph0, ph1);
    a.l1 = sr_gt_index<LOG2F>(t0 + 1, size, f, ph0, ph1);
    return a;
}

// Everything after the data-term gradient of one HR pixel: prior gradients and the optimiser update (shared by the
// fused and the gather backward kernels).  WTV: the TV branch takes (lambda_tv * w) of the edge each sign belongs to.
template <bool WTV>
__device__ __forceinline__ void sr_prior_and_update(const float* __restrict__ x, float* __restrict__ x_new, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ vhat,
                                                    const float* __restrict__ alphas, float* __restrict__ grad_out,
                                                    const SrDims& d, int b, int X, int Y, float g_df, float lambda_tv,
                                                    float two_lambda_l2, float lambda_l1, const SrStep& st,
                                                    const SrTvW& tw, float* __restrict__ x_bordered_out = nullptr) {
    const int H = d.H, W = d.W;
    // priors (superresolution.py:81-98): TV (forward differences, last row/col 0) or bilateral TV, L2, L1
    const float* img = x + (int64_t)b * H * W;
    const float xc = img[Y * W + X];
    auto sgn = [](float a) -> float { return (a > 0.0f) ? 1.0f : ((a < 0.0f) ? -1.0f : 0.0f); };
    float g_tv;
    if (st.prior == ASR_PRIOR_BTV) {
        // bilateral_tv (superresolution.py:8-23): sum over pairs p = (h, v), h in [-s, s], v in [0, s], of
        // alpha^(|h|+|v|) * || x - translate(x, p) ||_1 with translate(x, p)(q) = x(q - p), zero outside.
        // x enters twice: as the minuend (Abs grad = sign) and through the translate, whose registered gradient
        // samples the upstream at q + p.  Both sums run in the pair order of the reference's list comprehension.
        const int sh = st.btv_shift;
        float ga = 0.0f, gb = 0.0f;
        for (int hh = -sh; hh <= sh; ++hh)
            for (int vv = 0; vv <= sh; ++vv) {
                const float c = lambda_tv * st.btv_w[abs(hh) + vv];
                const int xs = X - hh, ys = Y - vv;
                const float sv = (xs >= 0 && xs < W && ys >= 0 && ys < H) ? img[ys * W + xs] : 0.0f;
                ga += sgn(xc - sv) * c;
            }
        for (int hh = -sh; hh <= sh; ++hh)
            for (int vv = 0; vv <= sh; ++vv) {
                const float c = lambda_tv * st.btv_w[abs(hh) + vv];
                const int xt = X + hh, yt = Y + vv;
                if (xt >= 0 && xt < W && yt >= 0 && yt < H) gb -= sgn(img[yt * W + xt] - xc) * c;
            }
        g_tv = ga + gb;
    } else if (WTV) {
        // four coalesced loads per pixel; the weights of the last row / column are never read
        const float* wyp = tw.wy + (int64_t)b * tw.stride;
        const float* wxp = tw.wx + (int64_t)b * tw.stride;
        const float sy = (Y < H - 1) ? sgn(img[(Y + 1) * W + X] - xc) * (lambda_tv * wyp[Y * W + X]) : 0.0f;
        const float sx = (X < W - 1) ? sgn(img[Y * W + X + 1] - xc) * (lambda_tv * wxp[Y * W + X]) : 0.0f;
        g_tv = -sy - sx;
        if (Y > 0) g_tv += sgn(xc - img[(Y - 1) * W + X]) * (lambda_tv * wyp[(Y - 1) * W + X]);
        if (X > 0) g_tv += sgn(xc - img[Y * W + X - 1]) * (lambda_tv * wxp[Y * W + X - 1]);
    } else {
        const float sy = (Y < H - 1) ? sgn(img[(Y + 1) * W + X] - xc) * lambda_tv : 0.0f;
        const float sx = (X < W - 1) ? sgn(img[Y * W + X + 1] - xc) * lambda_tv : 0.0f;
        g_tv = -sy - sx;
        if (Y > 0) g_tv += sgn(xc - img[(Y - 1) * W + X]) * lambda_tv;
        if (X > 0) g_tv += sgn(xc - img[Y * W + X - 1]) * lambda_tv;
    }
    float g = g_df + g_tv + two_lambda_l2 * xc;
    if (lambda_l1 > 0.0f) g = g + lambda_l1 * sgn(xc);

    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if (grad_out) grad_out[o] = g;
    if (!x_new) return;

    // apply_gradients: the dense CPU kernels of tensorflow/core/kernels/training_ops.cc that Keras 2.7 dispatches to
    // (operation order as in their Eigen expressions; alpha = the per-step scalar the host prepared)
    const float alpha = alphas[b];
    float xn;
    switch (st.optimizer) {
        case ASR_OPT_SGD: {                                 // ApplyGradientDescent / ApplyKerasMomentum
            if (st.c0 == 0.0f) {
                xn = xc - g * alpha;
            } else {
                const float acc = m[o] * st.c0 - g * alpha;
                m[o] = acc;
                xn = st.flag ? xc + (acc * st.c0 - g * alpha) : xc + acc;
            }
            break;
        }
        case ASR_OPT_ADAGRAD: {                             // ApplyAdagradV2
            const float acc = v[o] + g * g;
            v[o] = acc;
            xn = xc - (g * alpha) / (sqrtf(acc) + st.c2);
            break;
        }
        case ASR_OPT_ADADELTA: {                            // ApplyAdadelta: c0 = rho, c1 = 1 - rho
            const float acc = v[o] * st.c0 + (g * g) * st.c1;
            v[o] = acc;
            const float au = m[o];
            const float upd = sqrtf(au + st.c2) * (1.0f / sqrtf(acc + st.c2)) * g;
            xn = xc - upd * alpha;
            m[o] = au * st.c0 + (upd * upd) * st.c1;
            break;
        }
        case ASR_OPT_ADAMAX: {                              // ApplyAdaMax: c0 = 1 - beta1, c1 = beta2
            float mm = m[o];
            mm = mm + (g - mm) * st.c0;
            const float vv = fmaxf(st.c1 * v[o], fabsf(g));
            m[o] = mm;
            v[o] = vv;
            xn = xc - alpha * (mm / (vv + st.c2));
            break;
        }
        default: {                                          // ApplyAdam[WithAmsgrad]: c0 = 1 - beta1, c1 = 1 - beta2
            float mm = m[o], vv = v[o];
            mm = mm + (g - mm) * st.c0;
            vv = vv + (g * g - vv) * st.c1;
            m[o] = mm;
            v[o] = vv;
            float denom;
            if (st.flag) {
                const float vh = fmaxf(vhat[o], vv);
                vhat[o] = vh;
                denom = sqrtf(vh) + st.c2;
            } else {
                denom = sqrtf(vv) + st.c2;
            }
            xn = xc - (mm * alpha) / denom;
        }
    }
    x_new[o] = xn;
    if (x_bordered_out)   // the solver's zero-bordered copy for the next K_fwd
        x_bordered_out[(size_t)b * sr_gr_plane_elems(H, W) + (size_t)(Y + kGrPadY) * (W + 2 * kGrPadX) + (X + kGrPadX)] = xn;
}

// Work split: a workgroup owns 64 HR pixels (32 x 2) and NSPLIT = 4 waves; wave g evaluates the copies
// n = g, g + 4, ... for those pixels (the copy index is wave-uniform, so the transforms are scalar loads)
// and parks each contribution in LDS as contrib[n][pixel]; after one barrier wave 0 adds the N
// contributions IN COPY ORDER (the summation order of the oracle, so results stay bit-identical) and
// applies the priors and the Adam update.  4x the exposed parallelism of a one-thread-per-pixel loop for a
// latency-bound gather, N * 256 bytes of LDS.
constexpr int kBwdSplit = 4, kBwdPixX = 32, kBwdPixY = 2, kBwdPix = kBwdPixX * kBwdPixY;

// Two-kernel form of the data-term gradient (asr_sr_solve_*): G_R(n, c) -- the gradient that reaches the rotation stage
// at the integer HR position c of copy n, i.e. the registered gradient of the translate applied to G_T -- depends on
// (n, c) only, yet the fused kernel re-derives it for each of the 4 rotation taps of every (pixel, copy) pair (16 nested
// taps, ~250 VALU instructions per pair; the kernel is VALU-bound).  sr_grad_translate_kernel evaluates it ONCE per
// (n, c) into a zero-bordered [batch*n, H + 4, W + 64] plane (written and re-read through L2 / the Infinity Cache: 119 MB
// at N = 100, 512^2) and sr_backward_gather_kernel takes the rotation's 4 taps from that plane.  Same products and sums
// on the same operands as the fused kernel (x blend, then y blend, then the rotation's bilinear weights) -> bit-identical.
//   Plane geometry: row stride W + 64 (32 zero columns each side), 2 zero rows above and below.  A tap pair whose floor
//   coordinate is clamped to [-2, W] x [-2, H] reads only zeros wherever the unclamped taps are out of the image, so the
//   gather needs no per-tap bounds test and no select.
constexpr int kGrRows = 16;   // HR rows per wave of sr_grad_translate_kernel

// One wave: 64 columns x kGrRows rows of one copy.  The x taps are per lane (its column); the y taps of the wave's rows
// are computed by lanes 0..kGrRows-1 in ONE pass and fetched per row with v_readlane (they are wave-uniform: scalar row
// pointers, scalar validity branches).  The x blend of an LR row, h(L) = wl * G(L, l0) + wh * G(L, l1), serves the up
// to 4 HR rows that tap L: a two-entry cache keyed by the (uniform) LR row index keeps the last two.
template <int LOG2F, bool MON = false>
__global__ __launch_bounds__(256) void sr_grad_translate_kernel(const float* __restrict__ resid,
                                                                const float* __restrict__ inv_trans_tf,
                                                                float* __restrict__ gr_out, SrDims d, float two_lambda_df,
                                                                int n0, int cn, SrMonArg<MON> mon) {
    // blockIdx.z = b * cn + local: copy n0 + local of image b, written to plane slot blockIdx.z of the chunk's planes
    const int slot = blockIdx.z;
    if constexpr (MON) {
        if (mon.stopped[slot / cn]) return;      // a frozen image: its planes are never read again
    }
    const int bn = (slot / cn) * d.n + n0 + (slot % cn);
    const int lane = threadIdx.x;
    const int cx = blockIdx.x * 64 + lane;
    const int cy0 = (blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y)) * kGrRows;
    const int H = d.H, W = d.W, f = d.f, lw = d.w, lh = d.h;
    const int ph0 = f / 2 - 1, ph1 = f / 2;
    const int WP = W + 2 * kGrPadX;
    const float* r = resid + (int64_t)bn * lh * lw;
    const AsrTf8 it = asr_load_tf(inv_trans_tf + (int64_t)bn * 8);
    float* const out = gr_out + (size_t)slot * sr_gr_plane_elems(H, W) + (size_t)kGrPadY * WP + kGrPadX;
    const bool col_ok = cx < W;
    const bool pure_translation = (it.a0 == 1.0f && it.a1 == 0.0f && it.b0 == 0.0f && it.b1 == 1.0f &&
                                   it.c0 == 0.0f && it.c1 == 0.0f);
    if (pure_translation) {
        const SrAxisTap ax = sr_axis_tap<LOG2F>(col_ok ? cx : 0, it.a2, W, f, ph0, ph1);
        const int c0 = max(ax.l0, 0), c1 = max(ax.l1, 0);
        const bool ok0 = ax.l0 >= 0, ok1 = ax.l1 >= 0;
        const SrAxisTap ayv = sr_axis_tap<LOG2F>(min(cy0 + lane, H - 1), it.b2, H, f, ph0, ph1);   // lane j: row cy0 + j
        auto xblend = [&](int L) -> float {                         // L >= 0, wave-uniform
            const float* row = r + L * lw;
            const float a = (two_lambda_df * row[c0]) * 0.25f, b = (two_lambda_df * row[c1]) * 0.25f;
            return ax.wl * (ok0 ? a : 0.0f) + ax.wh * (ok1 ? b : 0.0f);
        };
        int la = -1, lb = -1;          // cached LR rows (lb the more recent)
        float va = 0.0f, vb = 0.0f;
        auto h_of = [&](int L) -> float {
            if (L < 0) return 0.0f;
            if (L == lb) return vb;
            if (L == la) return va;
            la = lb; va = vb;
            lb = L; vb = xblend(L);
            return vb;
        };
        const int rows = min(kGrRows, H - cy0);
        for (int j = 0; j < rows; ++j) {
            const float wl = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ayv.wl), j));
            const float wh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ayv.wh), j));
            const int l0 = __builtin_amdgcn_readlane(ayv.l0, j), l1 = __builtin_amdgcn_readlane(ayv.l1, j);
            const float h0 = h_of(l0), h1 = h_of(l1);
            if (col_ok) out[(cy0 + j) * WP + cx] = wl * h0 + wh * h1;
        }
    } else {   // generic projective inverse transforms (never produced by the reference's translate)
        auto gt_at = [&](int ly, int lx) -> float {
            const bool ok = (ly >= 0) & (lx >= 0);
            const float v = (two_lambda_df * r[ok ? ly * lw + lx : 0]) * 0.25f;
            return ok ? v : 0.0f;
        };
        auto rd_gt = [&](int yt, int xt) -> float {
            return gt_at(sr_gt_index<LOG2F>(yt, H, f, ph0, ph1), sr_gt_index<LOG2F>(xt, W, f, ph0, ph1));
        };
        for (int j = 0; j < kGrRows; ++j) {
            const int cy = cy0 + j;
            if (cy < H && col_ok) out[cy * WP + cx] = asr_tf_sample(it, rd_gt, cx, cy);
        }
    }
}

template <int LOG2F, bool WTV>
__global__ __launch_bounds__(256) void sr_backward_adam_kernel(
    const float* __restrict__ x, float* __restrict__ x_new, const float* __restrict__ resid,
    const float* __restrict__ inv_rot_tf, const float* __restrict__ inv_trans_tf,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
    const float* __restrict__ alphas /* [batch] for this iteration */, float* __restrict__ grad_out,
    SrDims d, float two_lambda_df, float lambda_tv, float two_lambda_l2, float lambda_l1, SrStep st, SrTvW tw) {
    extern __shared__ float contrib[];                     // [n][kBwdPix]
    const int X = blockIdx.x * kBwdPixX + threadIdx.x;
    const int Y = blockIdx.y * kBwdPixY + threadIdx.y;
    const int b = blockIdx.z;
    const int grp = threadIdx.z;                           // copy group == wave index
    const int pix = threadIdx.y * kBwdPixX + threadIdx.x;
    const bool in_image = (X < d.W) & (Y < d.H);
    const int H = d.H, W = d.W, f = d.f, lw = d.w, lh = d.h;
    const int ph0 = f / 2 - 1, ph1 = f / 2;

    // Two copies per trip: two independent instruction streams for the compiler to interleave (and to pair in packed
    // f32 math where it can) in a loop that is bound by VALU issue, not by memory.
    auto contribution = [&](int n) -> float {
        float g_df = 0.0f;
        const int bn = b * d.n + n;
        const AsrTf8 ir = asr_load_tf(inv_rot_tf + (int64_t)bn * 8);
        const float* r = resid + (int64_t)bn * lh * lw;
        const AsrTf8 it = asr_load_tf(inv_trans_tf + (int64_t)bn * 8);
        auto gt_at = [&](int ly, int lx) -> float {   // branch-free: clamped index, unconditional load, select
            const bool ok = (ly >= 0) & (lx >= 0);
            const float v = (two_lambda_df * r[ok ? ly * lw + lx : 0]) * 0.25f;
            return ok ? v : 0.0f;
        };
        const bool pure_translation = (it.a0 == 1.0f && it.a1 == 0.0f && it.b0 == 0.0f && it.b1 == 1.0f &&
                                       it.c0 == 0.0f && it.c1 == 0.0f);
        if (pure_translation) {
            // rotation stage (generic affine), then the separable translate stage
            float ix, iy;
            asr_tf_map(ir, (float)X, (float)Y, ix, iy);
            const float xf = floorf(ix), yf = floorf(iy);
            const int x0 = asr_coord_to_int(xf), y0 = asr_coord_to_int(yf);
            const SrAxisTap ax0 = sr_axis_tap<LOG2F>(x0, it.a2, W, f, ph0, ph1);
            const SrAxisTap ax1 = sr_axis_tap<LOG2F>(x0 + 1, it.a2, W, f, ph0, ph1);
            const SrAxisTap ay0 = sr_axis_tap<LOG2F>(y0, it.b2, H, f, ph0, ph1);
            const SrAxisTap ay1 = sr_axis_tap<LOG2F>(y0 + 1, it.b2, H, f, ph0, ph1);
            // The 4 x 4 G_T taps under this pixel sit on 3 consecutive HR positions per axis, i.e. on at most
            // 2 x 2 distinct LR residual cells: load those four values once and let every tap select its own
            // (16 gathers -> 4; the texture-address path, not the VALU, bounded this kernel).
            const int big = 0x3fffffff;
            auto lo_of = [&](int a, int b2, int c, int e) {
                return min(min(a >= 0 ? a : big, b2 >= 0 ? b2 : big), min(c >= 0 ? c : big, e >= 0 ? e : big));
            };
            const int cxa = lo_of(ax0.l0, ax0.l1, ax1.l0, ax1.l1), cxb = max(max(ax0.l0, ax0.l1), max(ax1.l0, ax1.l1));
            const int cya = lo_of(ay0.l0, ay0.l1, ay1.l0, ay1.l1), cyb = max(max(ay0.l0, ay0.l1), max(ay1.l0, ay1.l1));
            auto in2 = [](int l, int a, int b2) { return (l < 0) | (l == a) | (l == b2); };
            const bool two_cells = in2(ax0.l0, cxa, cxb) & in2(ax0.l1, cxa, cxb) & in2(ax1.l0, cxa, cxb) & in2(ax1.l1, cxa, cxb) &
                                   in2(ay0.l0, cya, cyb) & in2(ay0.l1, cya, cyb) & in2(ay1.l0, cya, cyb) & in2(ay1.l1, cya, cyb);
            const float wxl = (xf + 1.0f) - ix, wxh = ix - xf;
            if (two_cells) {
                const int xa = (cxa == big) ? 0 : cxa, xb = max(cxb, 0), ya = (cya == big) ? 0 : cya, yb = max(cyb, 0);
                const float saa = (two_lambda_df * r[ya * lw + xa]) * 0.25f, sab = (two_lambda_df * r[ya * lw + xb]) * 0.25f;
                const float sba = (two_lambda_df * r[yb * lw + xa]) * 0.25f, sbb = (two_lambda_df * r[yb * lw + xb]) * 0.25f;
                // The 16 taps select among the four cell values; selection and the x blend commute with the row choice,
                // so the x blend is done ONCE per (tap column pair, cell row) and the taps only pick a row afterwards --
                // the same products and sums on the same operands as tap-by-tap selection (an invalid tap contributes
                // w * 0 = +0 either way), a third of the v_cndmask / compare instructions this VALU-bound loop spent.
                auto cell = [&](int lx, float va, float vb) -> float {           // value of column lx in one cell row
                    const float v = (lx == cxa) ? va : vb;
                    return (lx >= 0) ? v : 0.0f;
                };
                auto hx = [&](const SrAxisTap& ax, float va, float vb) -> float {   // x blend of a tap column pair in one cell row
                    return ax.wl * cell(ax.l0, va, vb) + ax.wh * cell(ax.l1, va, vb);
                };
                const float h0a = hx(ax0, saa, sab), h0b = hx(ax0, sba, sbb);
                const float h1a = hx(ax1, saa, sab), h1b = hx(ax1, sba, sbb);
                auto row = [&](int ly, float ha, float hb) -> float {              // the x-blended value of tap row ly
                    const float v = (ly == cya) ? ha : hb;
                    return (ly >= 0) ? v : 0.0f;
                };
                auto gr = [&](const SrAxisTap& ay, const SrAxisTap& ax, float ha, float hb) -> float {   // G_R at one integer position
                    const float v = ay.wl * row(ay.l0, ha, hb) + ay.wh * row(ay.l1, ha, hb);
                    return (ay.inb & ax.inb) ? v : 0.0f;
                };
                const float vyf = wxl * gr(ay0, ax0, h0a, h0b) + wxh * gr(ay0, ax1, h1a, h1b);
                const float vyc = wxl * gr(ay1, ax0, h0a, h0b) + wxh * gr(ay1, ax1, h1a, h1b);
                g_df += ((yf + 1.0f) - iy) * vyf + (iy - yf) * vyc;
            } else {   // > 2 distinct cells on an axis: only through float rounding at a binade edge; 16 direct gathers
                auto gr = [&](const SrAxisTap& ay, const SrAxisTap& ax) -> float {
                    const float vyf = ax.wl * gt_at(ay.l0, ax.l0) + ax.wh * gt_at(ay.l0, ax.l1);
                    const float vyc = ax.wl * gt_at(ay.l1, ax.l0) + ax.wh * gt_at(ay.l1, ax.l1);
                    const float v = ay.wl * vyf + ay.wh * vyc;
                    return (ay.inb & ax.inb) ? v : 0.0f;
                };
                const float vyf = wxl * gr(ay0, ax0) + wxh * gr(ay0, ax1);
                const float vyc = wxl * gr(ay1, ax0) + wxh * gr(ay1, ax1);
                g_df += ((yf + 1.0f) - iy) * vyf + (iy - yf) * vyc;
            }
        } else {
            // generic projective inverse transforms (never produced by the reference's translate)
            auto rd_gt = [&](int yt, int xt) -> float {
                return gt_at(sr_gt_index<LOG2F>(yt, H, f, ph0, ph1), sr_gt_index<LOG2F>(xt, W, f, ph0, ph1));
            };
            auto rd_gr = [&](int yr, int xr) -> float {
                if (!(yr >= 0 && yr < H && xr >= 0 && xr < W)) return 0.0f;
                return asr_tf_sample(it, rd_gt, xr, yr);
            };
            g_df += asr_tf_sample(ir, rd_gr, X, Y);
        }
        return g_df;
    };
    int n = grp;
    for (; n + kBwdSplit < d.n; n += 2 * kBwdSplit) {
        const float g0 = contribution(n), g1 = contribution(n + kBwdSplit);
        contrib[n * kBwdPix + pix] = g0;
        contrib[(n + kBwdSplit) * kBwdPix + pix] = g1;
    }
    if (n < d.n) contrib[n * kBwdPix + pix] = contribution(n);
    __syncthreads();
    if (grp != 0 || !in_image) return;
    float g_df = 0.0f;
    for (int n = 0; n < d.n; ++n) g_df += contrib[n * kBwdPix + pix];   // fixed order n = 0..N-1

    sr_prior_and_update<WTV>(x, x_new, m, v, vhat, alphas, grad_out, d, b, X, Y, g_df, lambda_tv, two_lambda_l2, lambda_l1, st, tw);
}

// Backward, gather form: one thread per HR pixel walks the copies in order (the oracle's summation order) and takes
// the rotation's 2 x 2 taps of copy n from the zero-bordered G_R plane: two unaligned 8-byte loads, no bounds tests.
// The copy index is uniform, so the transforms are scalar loads.  The copies are taken K at a time: when all K rotations
// are affine (always, for the reference) the chunk is branch-free, so its 2K loads are in flight together and only the
// final adds are a dependent chain.
template <int K, bool AFFINE>
__device__ __forceinline__ float sr_gather_chunk(float g_df, const float* __restrict__ inv_rot_tf, const float* __restrict__ planes,
                                                 size_t plane, int WP, int H, int W, float fx, float fy) {
    AsrTf8 t[K];
#pragma unroll
    for (int u = 0; u < K; ++u) t[u] = asr_load_tf(inv_rot_tf + u * 8);
    float c[K];
    if (AFFINE) {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            float ix, iy;
            sr_map_affine(t[u], fx, fy, ix, iy);
            c[u] = sr_bilinear_bordered(planes + u * plane, WP, H, W, ix, iy);
        }
    } else {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            float ix, iy;
            c[u] = asr_tf_map(t[u], fx, fy, ix, iy) ? sr_bilinear_bordered(planes + u * plane, WP, H, W, ix, iy) : 0.0f;
        }
    }
#pragma unroll
    for (int u = 0; u < K; ++u) g_df += c[u];
    return g_df;
}

// flags[b] = 1 when every inverse rotation of image b is affine (c0 == c1 == 0: always, for the reference).  Evaluated once
// per solve -- the transforms do not change between the iterations -- instead of by every wave for every chunk of copies
// (two vector compares per copy and pixel in a kernel that is bound by VALU issue).
__global__ __launch_bounds__(64) void sr_affine_flags_kernel(const float* __restrict__ inv_rot_tf, int* __restrict__ flags, int n) {
    const int b = blockIdx.x;
    bool ok = true;
    for (int i = threadIdx.x; i < n; i += 64) {
        const float* t = inv_rot_tf + ((int64_t)b * n + i) * 8;
        ok = ok && t[6] == 0.0f && t[7] == 0.0f;
    }
    const bool all = __builtin_amdgcn_ballot_w64(!ok) == 0;
    if (threadIdx.x == 0) flags[b] = all ? 1 : 0;
}

// The data-term gradient of HR pixel (X, Y) of image b after the copies [n0, n0 + cn) of a chunk: the running sum of the chunks
// before (acc; +0 for the first) plus this chunk's rotation taps, in copy order: the gather of sr_backward_gather_kernel below,
// statement for statement, for the primal-dual kernel (that kernel keeps its own text: factored out, its machine code moved).
__device__ __forceinline__ float sr_gather_copies(const float* __restrict__ gr_planes, const float* __restrict__ inv_rot_tf,
                                                  const float* __restrict__ acc, const int* __restrict__ affine_flags,
                                                  const SrDims& d, int b, int X, int Y, int64_t o, int n0, int cn) {
    const int H = d.H, W = d.W, WP = W + 2 * kGrPadX;
    const size_t plane = sr_gr_plane_elems(H, W);
    const float* const planes = gr_planes + (size_t)b * cn * plane;
    const float* const tfs = inv_rot_tf + ((int64_t)b * d.n + n0) * 8;
    const float fx = (float)X, fy = (float)Y;
    float g_df = (n0 == 0) ? 0.0f : acc[o];
    int n = 0;
    if (affine_flags[b]) {       // the copies K at a time, branch-free: 2 K loads in flight, only the final adds are a chain
        for (; n + 8 <= cn; n += 8) g_df = sr_gather_chunk<8, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
        if (n + 4 <= cn) { g_df = sr_gather_chunk<4, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy); n += 4; }
        for (; n < cn; ++n) g_df = sr_gather_chunk<1, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
    } else {
        for (; n < cn; ++n) g_df = sr_gather_chunk<1, false>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
    }
    return g_df;
}

// ---- primal-dual update (ASR_OPT_PRIMAL_DUAL; include/asr_hip.h, "primal-dual": the rule, statement for statement) --------
// py / px: the dual planes before the iteration, py_new / px_new: after it -- other buffers, because a pixel rebuilds the new
// duals of its upper and left neighbours from their OLD values (a Jacobi step: nothing read here is written in this launch).
struct SrPd {
    const float* py;          // [batch, H, W]: the dual of the jump (Y,X) -> (Y+1,X)
    const float* px;          //                the dual of the jump (Y,X) -> (Y,X+1)
    float* py_new;
    float* px_new;
    float dual_ratio;         // cfg->c0: sigma = dual_ratio / tau
};

template <bool WTV>
__device__ __forceinline__ void sr_pd_update(const float* __restrict__ x, float* __restrict__ x_new, const SrPd& pd,
                                             const float* __restrict__ alphas, const SrDims& d, int b, int X, int Y, float g_df,
                                             float lambda_tv, float two_lambda_l2, float lambda_l1, const SrTvW& tw,
                                             float* __restrict__ x_bordered_out) {
    const int H = d.H, W = d.W;
    const int64_t img_o = (int64_t)b * H * W;
    const float* img = x + img_o;
    const float* pyo = pd.py + img_o;
    const float* pxo = pd.px + img_o;
    const int p = Y * W + X;
    const float xc = img[p];
    const float tau = alphas[b];
    const float sigma = pd.dual_ratio / tau;
    // the box of each dual: lambda_tv, or (lambda_tv * w) of the edge it belongs to
    float by = lambda_tv, bx = lambda_tv, by_up = lambda_tv, bx_left = lambda_tv;
    if (WTV) {
        const float* wyp = tw.wy + (int64_t)b * tw.stride;
        const float* wxp = tw.wx + (int64_t)b * tw.stride;
        by = lambda_tv * wyp[p];
        bx = lambda_tv * wxp[p];
        if (Y > 0) by_up = lambda_tv * wyp[p - W];
        if (X > 0) bx_left = lambda_tv * wxp[p - 1];
    }
    const float dY = (Y < H - 1) ? img[p + W] - xc : 0.0f;
    const float dX = (X < W - 1) ? img[p + 1] - xc : 0.0f;
    const float py0 = pyo[p], px0 = pxo[p];
    const float py1 = fminf(fmaxf(py0 + sigma * dY, -by), by);
    const float px1 = fminf(fmaxf(px0 + sigma * dX, -bx), bx);
    const float qy = 2.0f * py1 - py0;
    const float qx = 2.0f * px1 - px0;
    float div = -qy - qx;
    if (Y > 0) {                                   // the upper neighbour's new dual, from its old one
        const float pu0 = pyo[p - W];
        const float pu1 = fminf(fmaxf(pu0 + sigma * (xc - img[p - W]), -by_up), by_up);
        div += 2.0f * pu1 - pu0;
    }
    if (X > 0) {                                   // the left neighbour's
        const float pl0 = pxo[p - 1];
        const float pl1 = fminf(fmaxf(pl0 + sigma * (xc - img[p - 1]), -bx_left), bx_left);
        div += 2.0f * pl1 - pl0;
    }
    const float g = g_df + div + two_lambda_l2 * xc;
    const float u = xc - g * tau;
    float xn = u;
    if (lambda_l1 > 0.0f) {
        const float t = tau * lambda_l1;
        xn = (u > t) ? u - t : ((u < -t) ? u + t : 0.0f);
    }
    const int64_t o = img_o + p;
    pd.py_new[o] = py1;
    pd.px_new[o] = px1;
    x_new[o] = xn;
    x_bordered_out[(size_t)b * sr_gr_plane_elems(H, W) + (size_t)(Y + kGrPadY) * (W + 2 * kGrPadX) + (X + kGrPadX)] = xn;
}

// sr_backward_gather_kernel with the primal-dual update in the last chunk.  MON: a frozen image's workgroups carry x AND both
// dual planes over to the other buffers, and touch nothing else.
template <bool WTV, bool MON = false>
__global__ __launch_bounds__(256) void sr_backward_gather_pd_kernel(
    const float* __restrict__ x, float* __restrict__ x_new, const float* __restrict__ gr_planes,
    const float* __restrict__ inv_rot_tf, SrPd pd, const float* __restrict__ alphas, SrDims d, float lambda_tv,
    float two_lambda_l2, float lambda_l1, float* __restrict__ x_bordered_out, float* __restrict__ acc, int n0, int cn,
    const int* __restrict__ affine_flags, SrTvW tw, SrMonArg<MON> mon) {
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
    const float g_df = sr_gather_copies(gr_planes, inv_rot_tf, acc, affine_flags, d, b, X, Y, o, n0, cn);
    if (n0 + cn < d.n) { acc[o] = g_df; return; }
    sr_pd_update<WTV>(x, x_new, pd, alphas, d, b, X, Y, g_df, lambda_tv, two_lambda_l2, lambda_l1, tw, x_bordered_out);
}

// The copies are taken in chunks [n0, n0 + cn) (one launch per chunk, the chunk's planes written by the K_gt launch before
// it): the running sum of the data-term gradient crosses the launches through `acc` [batch, H, W] as a float32 -- the same
// sequence of float32 additions, in copy order, as one pass over all copies, so the result does not depend on the chunking.
// The last chunk adds the priors and applies the update.
// MON: a frozen image's workgroups carry x over to the other ping-pong buffer (in the chunk that would have applied the update)
// and touch nothing else -- not m, v, vhat, the bordered copy (it already holds this x) or acc.
template <bool WTV, bool MON = false>
__global__ __launch_bounds__(256) void sr_backward_gather_kernel(
    const float* __restrict__ x, float* __restrict__ x_new, const float* __restrict__ gr_planes,
    const float* __restrict__ inv_rot_tf, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
    const float* __restrict__ alphas, float* __restrict__ grad_out, SrDims d, float lambda_tv, float two_lambda_l2,
    float lambda_l1, SrStep st, float* __restrict__ x_bordered_out, float* __restrict__ acc, int n0, int cn,
    const int* __restrict__ affine_flags, SrTvW tw, SrMonArg<MON> mon) {
    const int X = blockIdx.x * 64 + threadIdx.x;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    const int H = d.H, W = d.W, WP = W + 2 * kGrPadX;
    if (X >= W || Y >= H) return;
    if constexpr (MON) {
        if (mon.stopped[b]) {
            if (n0 + cn >= d.n) {
                const int64_t oo = ((int64_t)b * H + Y) * W + X;
                x_new[oo] = x[oo];
            }
            return;
        }
    }
    const size_t plane = sr_gr_plane_elems(H, W);
    const float* const planes = gr_planes + (size_t)b * cn * plane;
    const float* const tfs = inv_rot_tf + ((int64_t)b * d.n + n0) * 8;
    const float fx = (float)X, fy = (float)Y;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    float g_df = (n0 == 0) ? 0.0f : acc[o];
    int n = 0;
    if (affine_flags[b]) {       // the copies K at a time, branch-free: 2 K loads in flight, only the final adds are a chain
        for (; n + 8 <= cn; n += 8) g_df = sr_gather_chunk<8, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
        if (n + 4 <= cn) { g_df = sr_gather_chunk<4, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy); n += 4; }
        for (; n < cn; ++n) g_df = sr_gather_chunk<1, true>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
    } else {
        for (; n < cn; ++n) g_df = sr_gather_chunk<1, false>(g_df, tfs + n * 8, planes + n * plane, plane, WP, H, W, fx, fy);
    }
    if (n0 + cn < d.n) { acc[o] = g_df; return; }
    sr_prior_and_update<WTV>(x, x_new, m, v, vhat, alphas, grad_out, d, b, X, Y, g_df, lambda_tv, two_lambda_l2, lambda_l1, st,
                             tw, x_bordered_out);
}

typedef void (*SrBwdKernel)(const float*, float*, const float*, const float*, const float*, float*, float*, float*,
                            const float*, float*, SrDims, float, float, float, float, SrStep, SrTvW);

template <bool WTV>
SrBwdKernel sr_backward_kernel_of(int f) {
    switch (f) {
        case 2: return sr_backward_adam_kernel<1, WTV>;
        case 4: return sr_backward_adam_kernel<2, WTV>;
        case 8: return sr_backward_adam_kernel<3, WTV>;
        default: return sr_backward_adam_kernel<0, WTV>;   // any other even factor: integer division
    }
}
SrBwdKernel sr_backward_kernel_for(int f, bool wtv) { return wtv ? sr_backward_kernel_of<true>(f) : sr_backward_kernel_of<false>(f); }

typedef void (*SrGradTranslateKernel)(const float*, const float*, float*, SrDims, float, int, int, SrMonArg<false>);
SrGradTranslateKernel sr_grad_translate_kernel_for(int f) {
    switch (f) {
        case 2: return sr_grad_translate_kernel<1>;
        case 4: return sr_grad_translate_kernel<2>;
        case 8: return sr_grad_translate_kernel<3>;
        default: return sr_grad_translate_kernel<0>;
    }
}
typedef void (*SrGradTranslateMonKernel)(const float*, const float*, float*, SrDims, float, int, int, SrMonArg<true>);
SrGradTranslateMonKernel sr_grad_translate_mon_kernel_for(int f) {
    switch (f) {
        case 2: return sr_grad_translate_kernel<1, true>;
        case 4: return sr_grad_translate_kernel<2, true>;
        case 8: return sr_grad_translate_kernel<3, true>;
        default: return sr_grad_translate_kernel<0, true>;
    }
}

// ---- loss terms (reporting only): out[b] = {df, tv, l2, l1} in float64 -------------------------
__global__ __launch_bounds__(256) void sr_loss_df_kernel(const float* __restrict__ resid, double* __restrict__ out,
                                                         int64_t per_image) {
    const int b = blockIdx.y;
    const float* r = resid + (int64_t)b * per_image;
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < per_image; p += (int64_t)gridDim.x * 256) {
        const float t = r[p];
        acc += (double)(t * t);
    }
    acc = asr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + (int64_t)b * 4 + 0, acc);
}

// terms[b][0] of a data term: sum w * rho(r) from the RAW residual.  Each term in float32, one operation per statement (at most
// four roundings: the Huber tail's subtraction and product, and the weight), accumulated in float64 like the sum above.
__global__ __launch_bounds__(256) void sr_loss_df_dt_kernel(const float* __restrict__ resid, double* __restrict__ out,
                                                            int64_t per_image, SrDt dt) {
    const int b = blockIdx.y;
    const float* r = resid + (int64_t)b * per_image;
    const float* wgt = dt.w ? dt.w + (int64_t)b * dt.w_stride : nullptr;
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < per_image; p += (int64_t)gridDim.x * 256) {
        const float t = r[p];
        const float a = fabsf(t);
        float rho;
        if (dt.loss == ASR_DF_L1) {
            rho = a;
        } else if (dt.loss == ASR_DF_HUBER && !(a <= dt.delta)) {
            const float lin = 2.0f * a - dt.delta;      // 2|r| is exact
            rho = dt.delta * lin;
        } else {
            rho = t * t;
        }
        if (wgt) rho = wgt[p] * rho;
        acc += (double)rho;
    }
    acc = asr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + (int64_t)b * 4 + 0, acc);
}

template <bool WTV>
__global__ __launch_bounds__(256) void sr_loss_prior_kernel(const float* __restrict__ x, double* __restrict__ out,
                                                            int H, int W, SrStep st, SrTvW tw) {
    const int b = blockIdx.y;
    const float* img = x + (int64_t)b * H * W;
    double tv = 0.0, l2 = 0.0, l1 = 0.0;
    const int64_t total = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        const int X = (int)(p % W), Y = (int)(p / W);
        const float xc = img[p];
        if (st.prior == ASR_PRIOR_BTV) {
            for (int hh = -st.btv_shift; hh <= st.btv_shift; ++hh)
                for (int vv = 0; vv <= st.btv_shift; ++vv) {
                    const int xs = X - hh, ys = Y - vv;
                    const float sv = (xs >= 0 && xs < W && ys >= 0 && ys < H) ? img[(int64_t)ys * W + xs] : 0.0f;
                    tv += (double)st.btv_w[abs(hh) + vv] * (double)fabsf(xc - sv);
                }
        } else if (WTV) {
            const float dy = (Y < H - 1) ? img[p + W] - xc : 0.0f;
            const float dx = (X < W - 1) ? img[p + 1] - xc : 0.0f;
            const int64_t q = (int64_t)b * tw.stride + p;      // the last row / column: weight read, times |0|
            tv += (double)(tw.wy[q] * fabsf(dy) + tw.wx[q] * fabsf(dx));
        } else {
            const float dy = (Y < H - 1) ? img[p + W] - xc : 0.0f;
            const float dx = (X < W - 1) ? img[p + 1] - xc : 0.0f;
            tv += (double)(fabsf(dy) + fabsf(dx));
        }
        l2 += (double)(xc * xc);
        l1 += (double)fabsf(xc);
    }
    tv = asr_wave_sum(tv);
    l2 = asr_wave_sum(l2);
    l1 = asr_wave_sum(l1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(out + (int64_t)b * 4 + 1, tv);
        atomicAdd(out + (int64_t)b * 4 + 2, l2);
        atomicAdd(out + (int64_t)b * 4 + 3, l1);
    }
}

// ---- realign: max / mean / order statistics over copies of InvWarp(upsample(y_n)) (superresolution.py:139-161) --
// NP values that go through the per-copy arithmetic side by side: plane p of a copy sampled at ONE set of coordinates with
// ONE set of weights.  The operators are element-wise, each the single f32 operation it spells, so every plane's value is
// what the same statements give on floats (NP = 1 IS a float).
template <int NP>
struct SrPlanes {
    float v[NP];
};
template <int NP>
__device__ __forceinline__ SrPlanes<NP> operator+(const SrPlanes<NP>& a, const SrPlanes<NP>& b) {
    SrPlanes<NP> r;
#pragma unroll
    for (int p = 0; p < NP; ++p) r.v[p] = a.v[p] + b.v[p];
    return r;
}
template <int NP>
__device__ __forceinline__ SrPlanes<NP> operator-(const SrPlanes<NP>& a, const SrPlanes<NP>& b) {
    SrPlanes<NP> r;
#pragma unroll
    for (int p = 0; p < NP; ++p) r.v[p] = a.v[p] - b.v[p];
    return r;
}
template <int NP>
__device__ __forceinline__ SrPlanes<NP> operator*(const SrPlanes<NP>& a, float s) {
    SrPlanes<NP> r;
#pragma unroll
    for (int p = 0; p < NP; ++p) r.v[p] = a.v[p] * s;
    return r;
}
template <int NP>
__device__ __forceinline__ SrPlanes<NP> operator*(float s, const SrPlanes<NP>& a) {
    SrPlanes<NP> r;
#pragma unroll
    for (int p = 0; p < NP; ++p) r.v[p] = s * a.v[p];
    return r;
}

// The value of copy bn = b * n + i at output pixel (X, Y): rotate(translate(resize(y[bn], (H,W)), trans_tf[bn]), rot_tf[bn]),
// zero fill included.  The ONE statement of that arithmetic: sr_realign_kernel folds it into a max / a sum,
// sr_realign_select_kernel selects from it, and the covered kernels take it for the copy's plane of y (.v[0], src[0]) AND
// for its weight plane (.v[1], src[1]) -- the geometry (both coordinate maps, floors, tap weights, in-frame tests, the choice
// of the fast path) is computed once and serves every plane -- so all of them agree bit for bit.  src[p]: plane p of THIS copy.
template <int NP>
__device__ __forceinline__ SrPlanes<NP> sr_realign_copy_value(const float* const (&src)[NP], const float* __restrict__ trans_tf,
                                                              const float* __restrict__ rot_tf, int bn, int X, int Y, int H, int W,
                                                              int lh, int lw, float scale_y, float scale_x) {
    typedef SrPlanes<NP> V;
    const V zero = {};
    const AsrTf8 tt = asr_load_tf(trans_tf + (int64_t)bn * 8);
    const AsrTf8 tr = asr_load_tf(rot_tf + (int64_t)bn * 8);
    auto rd_up = [&](int yu, int xu) -> V {  // tf.image.resize(y_n, (H,W)) at integer (yu,xu)
        if (!(yu >= 0 && yu < H && xu >= 0 && xu < W)) return zero;
        const AsrLerp ly = asr_half_pixel(yu, scale_y, lh);
        const AsrLerp lx = asr_half_pixel(xu, scale_x, lw);
        V tl, trv, bl, br;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            tl.v[p] = src[p][ly.lo * lw + lx.lo]; trv.v[p] = src[p][ly.lo * lw + lx.hi];
            bl.v[p] = src[p][ly.hi * lw + lx.lo]; br.v[p] = src[p][ly.hi * lw + lx.hi];
        }
        const V top = tl + (trv - tl) * lx.t;
        const V bot = bl + (br - bl) * lx.t;
        return top + (bot - top) * ly.t;
    };
    auto rd_tr = [&](int yt, int xt) -> V {
        if (!(yt >= 0 && yt < H && xt >= 0 && xt < W)) return zero;
        return asr_tf_sample(tt, rd_up, xt, yt);
    };
    V val;
    // Pure translation (always, for tfa.image.translate): the 2 x 2 translate-stage pixels under the rotation sample
    // read a 3 x 3 block of upsampled pixels (2 x 2 taps each, shifted by one); evaluate those 9 resize samples once
    // instead of 16 times.  Same per-tap arithmetic as the generic path (bit-identical); the generic path stays for
    // other transforms and for the float-rounding case where the two tap columns / rows do not abut.
    float ix, iy;
    const bool ok = asr_tf_map(tr, (float)X, (float)Y, ix, iy);
    const float xf = floorf(ix), yf = floorf(iy);
    const int x0 = asr_coord_to_int(xf), y0 = asr_coord_to_int(yf);
    const bool pure_translation = (tt.a0 == 1.0f) & (tt.a1 == 0.0f) & (tt.b0 == 0.0f) & (tt.b1 == 1.0f) &
                                  (tt.c0 == 0.0f) & (tt.c1 == 0.0f);
    const float jx0 = (float)x0 + tt.a2, jx1 = (float)(x0 + 1) + tt.a2;
    const float jy0 = (float)y0 + tt.b2, jy1 = (float)(y0 + 1) + tt.b2;
    const float fx0 = floorf(jx0), fx1 = floorf(jx1), fy0 = floorf(jy0), fy1 = floorf(jy1);
    const int cx0 = asr_coord_to_int(fx0), cx1 = asr_coord_to_int(fx1);
    const int cy0 = asr_coord_to_int(fy0), cy1 = asr_coord_to_int(fy1);
    if (ok && pure_translation && cx1 == cx0 + 1 && cy1 == cy0 + 1) {
        V uv[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) uv[a][c] = rd_up(cy0 + a, cx0 + c);
        const float wxl0 = (fx0 + 1.0f) - jx0, wxh0 = jx0 - fx0, wxl1 = (fx1 + 1.0f) - jx1, wxh1 = jx1 - fx1;
        const float wyl0 = (fy0 + 1.0f) - jy0, wyh0 = jy0 - fy0, wyl1 = (fy1 + 1.0f) - jy1, wyh1 = jy1 - fy1;
        auto Tq = [&](int a, int c, float wxl, float wxh, float wyl, float wyh) -> V {
            const V vyf = wxl * uv[a][c] + wxh * uv[a][c + 1];
            const V vyc = wxl * uv[a + 1][c] + wxh * uv[a + 1][c + 1];
            return wyl * vyf + wyh * vyc;
        };
        const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
        const V v00 = (vy0 && vx0) ? Tq(0, 0, wxl0, wxh0, wyl0, wyh0) : zero;
        const V v01 = (vy0 && vx1) ? Tq(0, 1, wxl1, wxh1, wyl0, wyh0) : zero;
        const V v10 = (vy1 && vx0) ? Tq(1, 0, wxl0, wxh0, wyl1, wyh1) : zero;
        const V v11 = (vy1 && vx1) ? Tq(1, 1, wxl1, wxh1, wyl1, wyh1) : zero;
        const float wxl = (xf + 1.0f) - ix, wxh = ix - xf;
        const V vyf = wxl * v00 + wxh * v01;
        const V vyc = wxl * v10 + wxh * v11;
        val = ((yf + 1.0f) - iy) * vyf + (iy - yf) * vyc;
    } else {
        val = asr_tf_sample(tr, rd_tr, X, Y);
    }
    return val;
}
// the one-plane form: plane bn of y
__device__ __forceinline__ float sr_realign_copy_value(const float* __restrict__ y, const float* __restrict__ trans_tf,
                                                       const float* __restrict__ rot_tf, int bn, int X, int Y, int H, int W,
                                                       int lh, int lw, float scale_y, float scale_x) {
    const float* const src[1] = {y + (int64_t)bn * lh * lw};
    return sr_realign_copy_value<1>(src, trans_tf, rot_tf, bn, X, Y, H, W, lh, lw, scale_y, scale_x).v[0];
}

// MODE 0: mean -> out_a; 1: max -> out_a; 2: both in one pass (max -> out_a, mean -> out_b): the reference calls
// max_superresolution and mean_superresolution on the same copies (SR_single_class.py:103-110), and the per-copy value
// is the expensive part.
template <int MODE>
__global__ __launch_bounds__(256) void sr_realign_kernel(const float* __restrict__ y, float* __restrict__ out_a,
                                                         float* __restrict__ out_b,
                                                         const float* __restrict__ trans_tf /* translate(-s) */,
                                                         const float* __restrict__ rot_tf /* rotate(-theta) */,
                                                         SrDims d, float scale_y, float scale_x) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const int H = d.H, W = d.W, lh = d.h, lw = d.w;
    float acc_sum = 0.0f, acc_max = 0.0f;
    for (int n = 0; n < d.n; ++n) {
        const float val = sr_realign_copy_value(y, trans_tf, rot_tf, b * d.n + n, X, Y, H, W, lh, lw, scale_y, scale_x);
        if (MODE != 0) acc_max = (n == 0) ? val : fmaxf(acc_max, val);
        if (MODE != 1) acc_sum += val;
    }
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if (MODE == 0) out_a[o] = acc_sum / (float)d.n;
    if (MODE == 1) out_a[o] = acc_max;
    if (MODE == 2) { out_a[o] = acc_max; out_b[o] = acc_sum / (float)d.n; }
}

// ---- order statistics over the same copies: quantiles and the trimmed mean (include/asr_hip.h: the rule) --------------
// One thread per output pixel, one wave per workgroup (32 x 2 pixels).  The thread parks its n per-copy values in LDS as
// [copy][pixel], pixel fastest: lane l only ever touches dword l of a 64-dword row, so a column walks ONE bank, no two
// lanes share a bank, and no barrier is needed (nobody reads another lane's column).  256 bytes per copy: 25.6 KB at
// n = 100, 51.2 KB at n = 200, 160 KiB at the cap of 640 copies; LDS, not registers, bounds the waves per CU (640 / n).
// The values are parked as order-preserving keys (sign bit flipped for x >= 0, all bits for x < 0; -0 parked as +0), so
// every comparison below is one unsigned compare.  s[rank] comes from a 32-step bisection on the key's bits: the largest
// p with #(key < p) <= rank IS the key of s[rank]; each step counts its column once, the update is a select -- no sort,
// no data-dependent branch, the same instruction stream for every lane.
constexpr int kSelX = 32, kSelY = 2, kSelPix = kSelX * kSelY;
constexpr int kSelMaxQ = 8;
constexpr int kSelLdsMax = 160 * 1024;
constexpr int kSelMaxCopies = kSelLdsMax / (kSelPix * (int)sizeof(unsigned));      // 640

struct SrSelect {
    int num_q, trim_k;
    int lo[kSelMaxQ], hi[kSelMaxQ];
    float t[kSelMaxQ];
};

__device__ __forceinline__ unsigned sr_sel_key(float v) {
    const unsigned u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float sr_sel_value(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
// key of s[rank], 0 <= rank < n; col: this lane's column (stride kSelPix)
__device__ __forceinline__ unsigned sr_sel_rank(const unsigned* col, int n, int rank) {
    unsigned prefix = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int below = 0;
#pragma unroll 8
        for (int i = 0; i < n; ++i) below += (col[i * kSelPix] < cand) ? 1 : 0;
        prefix = (below <= rank) ? cand : prefix;
    }
    return prefix;
}

__global__ __launch_bounds__(kSelPix) void sr_realign_select_kernel(const float* __restrict__ y, float* __restrict__ out_q,
                                                                    float* __restrict__ out_trim,
                                                                    const float* __restrict__ trans_tf,
                                                                    const float* __restrict__ rot_tf, SrDims d, SrSelect sel,
                                                                    int tiles_x, float scale_y, float scale_x) {
    extern __shared__ unsigned sel_keys[];                 // [n][kSelPix]
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int X = tile_x * kSelX + threadIdx.x;
    const int Y = tile_y * kSelY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const int H = d.H, W = d.W, lh = d.h, lw = d.w, n = d.n;
    unsigned* col = sel_keys + threadIdx.y * kSelX + threadIdx.x;
    for (int i = 0; i < n; ++i) {
        const float val = sr_realign_copy_value(y, trans_tf, rot_tf, b * n + i, X, Y, H, W, lh, lw, scale_y, scale_x);
        col[i * kSelPix] = sr_sel_key(val);
    }
    const int64_t plane = (int64_t)d.batch * H * W;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    for (int j = 0; j < sel.num_q; ++j) {
        const int lo = sel.lo[j], hi = sel.hi[j];
        const unsigned ka = sr_sel_rank(col, n, lo);
        float r = sr_sel_value(ka);
        if (hi != lo) {
            unsigned kb;
            if (hi == lo + 1) {
                // the next rank in one more pass: s[lo + 1] is s[lo] again while copies of it remain, else the least key above
                int le = 0;
                unsigned next = 0xffffffffu;
#pragma unroll 8
                for (int i = 0; i < n; ++i) {
                    const unsigned k = col[i * kSelPix];
                    le += (k <= ka) ? 1 : 0;
                    next = (k > ka && k < next) ? k : next;
                }
                kb = (hi < le) ? ka : next;
            } else {
                kb = sr_sel_rank(col, n, hi);
            }
            r = r + (sr_sel_value(kb) - r) * sel.t[j];
        }
        out_q[j * plane + o] = r;
    }
    if (out_trim) {
        const int k = sel.trim_k, m = n - 2 * k;
        const unsigned ka = sr_sel_rank(col, n, k);
        const unsigned kc = (m == 1) ? ka : sr_sel_rank(col, n, n - 1 - k);
        const float a = sr_sel_value(ka), c = sr_sel_value(kc);
        float sum = 0.0f;
        int le_a = 0, lt_c = 0;
#pragma unroll 8
        for (int i = 0; i < n; ++i) {                      // copy order
            const unsigned key = col[i * kSelPix];
            sum += (key > ka && key < kc) ? sr_sel_value(key) : 0.0f;
            le_a += (key <= ka) ? 1 : 0;
            lt_c += (key < kc) ? 1 : 0;
        }
        if (ka == kc) {
            sum = (float)m * a;
        } else {
            sum = sum + (float)(le_a - k) * a;             // the copies of a at ranks k ..
            sum = sum + (float)(n - k - lt_c) * c;         // the copies of c at ranks .. n - 1 - k
        }
        out_trim[o] = sum / (float)m;
    }
}

// ---- coverage-normalised fusions over the same copies (include/asr_hip.h: the rule) -----------------------------------
// Each copy's weight plane goes through the statements of its plane of y (sr_realign_copy_value<2>: one geometry, two
// planes); C = sum of the realigned weights, S = sum of the realigned values, both in copy order like acc_sum above.
// No packed f32 in these kernels: the unit's default is switched off for them (the two planes invite pairing, and the
// compiler picks op_sel by itself -- isa_guard.py).
#if defined(__HIP_DEVICE_COMPILE__)
#define SR_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SR_NO_PK_F32
#endif

struct SrCover {
    float cov_min, valid_min;
    int64_t wgt_stride;        // floats between the weight planes of two copies: lh * lw, or 0 for one shared plane
};

// Mean and / or coverage: the shape of sr_realign_kernel, registers only.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_realign_covered_kernel(
    const float* __restrict__ y, const float* __restrict__ wgt, float* __restrict__ out_mean, float* __restrict__ out_cov,
    const float* __restrict__ trans_tf, const float* __restrict__ rot_tf, SrDims d, SrCover cv, float scale_y, float scale_x) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const int H = d.H, W = d.W, lh = d.h, lw = d.w;
    float acc_sum = 0.0f, acc_cov = 0.0f;
    for (int n = 0; n < d.n; ++n) {
        const int bn = b * d.n + n;
        const float* const src[2] = {y + (int64_t)bn * lh * lw, wgt + (int64_t)bn * cv.wgt_stride};
        const SrPlanes<2> val = sr_realign_copy_value<2>(src, trans_tf, rot_tf, bn, X, Y, H, W, lh, lw, scale_y, scale_x);
        acc_sum += val.v[0];
        acc_cov += val.v[1];
    }
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if (out_cov) out_cov[o] = acc_cov;
    if (out_mean) out_mean[o] = (acc_cov >= cv.cov_min) ? acc_sum / acc_cov : 0.0f;
}

// With the median over the valid copies (c_i >= valid_min): the select kernel's LDS layout ([copy][pixel] keys, one wave per
// workgroup, no barrier) and its bisection.  An invalid copy is parked as 0xffffffff, above the key of every finite value
// (and of +inf), so the nv valid keys are the nv smallest of the column and s[rank], rank < nv, is found among all n; the
// ranks come from the pixel's own nv, and the even / odd and nv = 0 cases are selects.
__global__ __launch_bounds__(kSelPix) SR_NO_PK_F32 void sr_realign_covered_median_kernel(
    const float* __restrict__ y, const float* __restrict__ wgt, float* __restrict__ out_mean, float* __restrict__ out_median,
    float* __restrict__ out_cov, const float* __restrict__ trans_tf, const float* __restrict__ rot_tf, SrDims d, SrCover cv,
    int tiles_x, float scale_y, float scale_x) {
    extern __shared__ unsigned sel_keys[];                 // [n][kSelPix]
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int X = tile_x * kSelX + threadIdx.x;
    const int Y = tile_y * kSelY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const int H = d.H, W = d.W, lh = d.h, lw = d.w, n = d.n;
    unsigned* col = sel_keys + threadIdx.y * kSelX + threadIdx.x;
    float acc_sum = 0.0f, acc_cov = 0.0f;
    int nv = 0;
    for (int i = 0; i < n; ++i) {
        const int bn = b * n + i;
        const float* const src[2] = {y + (int64_t)bn * lh * lw, wgt + (int64_t)bn * cv.wgt_stride};
        const SrPlanes<2> val = sr_realign_copy_value<2>(src, trans_tf, rot_tf, bn, X, Y, H, W, lh, lw, scale_y, scale_x);
        acc_sum += val.v[0];
        acc_cov += val.v[1];
        const bool valid = val.v[1] >= cv.valid_min;
        nv += valid ? 1 : 0;
        col[i * kSelPix] = valid ? sr_sel_key(val.v[0]) : 0xffffffffu;
    }
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    if (out_cov) out_cov[o] = acc_cov;
    if (out_mean) out_mean[o] = (acc_cov >= cv.cov_min) ? acc_sum / acc_cov : 0.0f;
    const int lo = max(nv - 1, 0) / 2, hi = nv / 2;        // nv = 0: rank 0 of a column of parked keys, discarded below
    const unsigned ka = sr_sel_rank(col, n, lo);
    int le = 0;
    unsigned next = 0xffffffffu;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {                          // s[lo + 1]: s[lo] again while copies of it remain, else the least key above
        const unsigned k = col[i * kSelPix];
        le += (k <= ka) ? 1 : 0;
        next = (k > ka && k < next) ? k : next;
    }
    const unsigned kb = (hi < le) ? ka : next;
    const float a = sr_sel_value(ka);
    const float mid = a + (sr_sel_value(kb) - a) * 0.5f;
    const float r = (hi != lo) ? mid : a;
    out_median[o] = (nv > 0) ? r : 0.0f;
}

// ---- mean, population variance and valid count over the same copies (include/asr_hip.h: the rule) ----------------------
// The shape of sr_realign_covered_kernel, registers only, for any n: the copies are walked twice, first for the sum and the
// count of the valid ones (m = sum / nv), then for the squared deviations about that rounded m.  The second walk recomputes
// every v_i with the same statements (the taps come from the caches), so nothing is parked and n has no cap.  HAS_W = false:
// no weight plane, every copy is valid and the sum is sr_realign_kernel's own.  An invalid copy adds +0 to a sum that
// starts at +0, which leaves its bits alone.
template <bool HAS_W>
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_realign_moments_kernel(
    const float* __restrict__ y, const float* __restrict__ wgt, float* __restrict__ out_mean, float* __restrict__ out_var,
    float* __restrict__ out_nv, const float* __restrict__ trans_tf, const float* __restrict__ rot_tf, SrDims d, SrCover cv,
    float scale_y, float scale_x) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= d.W || Y >= d.H) return;
    const int H = d.H, W = d.W, lh = d.h, lw = d.w;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    const int walks = out_var ? 2 : 1;
    float m = 0.0f, fnv = 0.0f;
    // ONE textual walk, run once or twice: with a second inlined copy of sr_realign_copy_value the kernel took 192 bytes of
    // scratch per lane and 114 VGPRs (4 waves per SIMD, 6.8 x the time of one mean walk); this form has none and 64
#pragma nounroll
    for (int walk = 0; walk < walks; ++walk) {
        float acc = 0.0f;
        int cnt = 0;
        for (int n = 0; n < d.n; ++n) {
            const int bn = b * d.n + n;
            float v;
            bool valid = true;
            if (HAS_W) {
                const float* const src[2] = {y + (int64_t)bn * lh * lw, wgt + (int64_t)bn * cv.wgt_stride};
                const SrPlanes<2> val = sr_realign_copy_value<2>(src, trans_tf, rot_tf, bn, X, Y, H, W, lh, lw, scale_y, scale_x);
                v = val.v[0];
                valid = val.v[1] >= cv.valid_min;
            } else {
                v = sr_realign_copy_value(y, trans_tf, rot_tf, bn, X, Y, H, W, lh, lw, scale_y, scale_x);
            }
            const float dv = v - m;                            // the first walk has m = +0: dv is v, bit for bit
            const float term = walk ? dv * dv : dv;            // the product and the add round separately (-ffp-contract=off)
            acc += valid ? term : 0.0f;
            cnt += valid ? 1 : 0;
        }
        if (walk == 0) {
            fnv = (float)cnt;
            m = (cnt > 0) ? acc / fnv : 0.0f;
            if (out_nv) out_nv[o] = fnv;
            if (out_mean) out_mean[o] = m;
        } else {
            out_var[o] = (fnv > 0.0f) ? acc / fnv : 0.0f;
        }
    }
}

int check_dims(const char* fn, int batch, int n, int H, int W, int h, int w, SrDims* d) {
    ASR_REQUIRE(batch > 0 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "%s: bad shape batch=%d n=%d %dx%d <- %dx%d",
                fn, batch, n, H, W, h, w);
    ASR_REQUIRE((int64_t)batch * n <= 65535, "%s: batch*n=%lld exceeds 65535 (grid.z)", fn, (long long)batch * n);
    const int f = H / h;
    ASR_UNSUPPORTED(f * h != H || f * w != W || f < 2 || (f & 1),
                    "%s: output %dx%d must be an even integer multiple of the feature size %dx%d", fn, H, W, h, w);
    d->batch = batch; d->n = n; d->H = H; d->W = W; d->h = h; d->w = w; d->f = f;
    return ASR_OK;
}

int prepare_backward(const SrDims& d, bool wtv) {
    const size_t lds = sizeof(float) * (size_t)d.n * 64;
    ASR_UNSUPPORTED(lds > 160 * 1024, "asr_sr: num_aug=%d needs %zu bytes of LDS in the backward kernel (max 640 copies)", d.n, lds);
    static AsrDeviceOnce once[8];
    const int idx = (d.f == 2 ? 1 : (d.f == 4 ? 2 : (d.f == 8 ? 3 : 0))) + (wtv ? 4 : 0);
    if (lds > 64 * 1024)
        ASR_HIP_CHECK(asr_allow_dynamic_lds(once[idx], reinterpret_cast<const void*>(sr_backward_kernel_for(d.f, wtv)), 160 * 1024));
    return ASR_OK;
}
dim3 gr_grid(const SrDims& d, int cn) {
    return dim3((unsigned)asr_cdiv(d.W, 64), (unsigned)asr_cdiv(d.H, 4 * kGrRows), (unsigned)(d.batch * cn));
}
// Copies whose gradient planes are alive at once.  The planes (1.07 MB each at 512 x 512) are written by K_gt and read
// back by K_bwd in the same iteration: 107 MB at N = 100, 214 MB at N = 200.  Cutting them into chunks of <= 32 copies
// (<= 35 MB live) was measured SLOWER on every shape and lane count (profiles/r03_sr_plane_chunk_experiment.txt: N = 100
// 99 -> 127 us per iteration, N = 200 314 -> 348 us, two solves in flight 614 -> 694 us): each extra launch pair costs
// more than the Infinity Cache misses it avoids, and the fabric counters see the planes either way.  The library default
// therefore keeps all copies in one chunk while the planes stay under kPlaneBytesMax per call and splits evenly beyond
// (a bound on the workspace, not a speed-up); cfg->plane_chunk overrides.
constexpr size_t kPlaneBytesMax = (size_t)1 << 30;
int sr_plane_chunk(int batch, int n, int H, int W, int requested) {
    if (requested > 0) return requested < n ? requested : n;
    const size_t per_copy = sizeof(float) * (size_t)batch * sr_gr_plane_elems(H, W);
    const size_t fit = kPlaneBytesMax / per_copy > 0 ? kPlaneBytesMax / per_copy : 1;
    if ((size_t)n <= fit) return n;
    const int chunks = (int)(((size_t)n + fit - 1) / fit);
    return (n + chunks - 1) / chunks;
}
size_t sr_workspace_bytes(int batch, int n, int H, int W, int h, int w, int chunk) {
    // residuals [batch*n, h, w] + the ping-pong x [batch, H, W] + the running data-term sum [batch, H, W] + the
    // zero-bordered planes [H + 4, W + 64]: G_R per copy of a chunk, x per image
    // + one int per image: "all inverse rotations affine"
    return sizeof(float) * ((size_t)batch * n * h * w + 2 * (size_t)batch * H * W +
                            ((size_t)batch * chunk + batch) * sr_gr_plane_elems(H, W)) + sizeof(int) * (size_t)batch;
}
size_t sr_dt_workspace_extra(int batch, int n, int h, int w) { return sizeof(float) * (size_t)batch * n * h * w; }
dim3 gather_grid(const SrDims& d) {
    return dim3((unsigned)asr_cdiv(d.W, 64), (unsigned)asr_cdiv(d.H, 4), (unsigned)d.batch);
}
dim3 bwd_grid(const SrDims& d) { return dim3((unsigned)asr_cdiv(d.W, kBwdPixX), (unsigned)asr_cdiv(d.H, kBwdPixY), (unsigned)d.batch); }
const dim3 kBwdBlock(kBwdPixX, kBwdPixY, kBwdSplit);
size_t bwd_lds(const SrDims& d) { return sizeof(float) * (size_t)d.n * kBwdPix; }
dim3 hr_grid(const SrDims& d) { return dim3((unsigned)asr_cdiv(d.W, kTileX), (unsigned)asr_cdiv(d.H, kTileY), (unsigned)d.batch); }
dim3 lr_grid(const SrDims& d) { return dim3((unsigned)asr_cdiv(d.w, kTileX), (unsigned)asr_cdiv(d.h, kTileY), (unsigned)(d.batch * d.n)); }
const dim3 kBlock(kTileX, kTileY);

}  // namespace

extern "C" int asr_sr_init_target_f32(const float* y, float* x, int batch, int n, int H, int W, int h, int w,
                                      asr_stream_t stream) {
    ASR_REQUIRE(y && x, "asr_sr_init_target_f32: null pointer");
    SrDims d;
    ASR_REQUIRE(batch > 0 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "asr_sr_init_target_f32: bad shape");
    d.batch = batch; d.n = n; d.H = H; d.W = W; d.h = h; d.w = w; d.f = 0;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipLaunchKernelGGL(sr_init_kernel, hr_grid(d), kBlock, 0, asr_stream(stream), y, x, d, sy, sx);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_sr_forward_residual_f32(const float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                           float* resid, int batch, int n, int H, int W, int h, int w,
                                           asr_stream_t stream) {
    ASR_REQUIRE(x && y && rot_tf && trans_tf && resid, "asr_sr_forward_residual_f32: null pointer");
    SrDims d;
    int rc = check_dims("asr_sr_forward_residual_f32", batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(sr_forward_residual_kernel<false>, lr_grid(d), kBlock, 0, asr_stream(stream), x, y, rot_tf, trans_tf,
                       resid, d, SrDtArg<false>{}, SrMonArg<false>{});
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

namespace {

// asr_sr_data_term -> kernel argument and the TV planes; every refusal of the data term, before any launch.  n, h, w: the
// shape the weights are read with.
int make_data_term(const char* fn, const asr_sr_data_term* dt, int n, int h, int w, SrDt* out) {
    ASR_REQUIRE(dt, "%s: null data term", fn);
    ASR_REQUIRE(dt->loss == ASR_DF_L2 || dt->loss == ASR_DF_L1 || dt->loss == ASR_DF_HUBER, "%s: unknown loss %d", fn, dt->loss);
    if (dt->loss == ASR_DF_HUBER)
        ASR_REQUIRE(dt->delta > 0.0f && dt->delta < __builtin_inff(), "%s: Huber delta=%g must be finite and > 0", fn, (double)dt->delta);
    ASR_REQUIRE((dt->wy == nullptr) == (dt->wx == nullptr), "%s: null pointer (wy, wx: both or neither)", fn);
    if (dt->weights) ASR_REQUIRE(n > 0 && h > 0 && w > 0, "%s: weights with a bad shape n=%d %dx%d", fn, n, h, w);
    out->loss = dt->loss;
    out->delta = dt->delta;
    out->w = dt->weights;
    out->w_stride = dt->weights_shared ? 0 : (int64_t)n * h * w;
    out->r_out = nullptr;
    return ASR_OK;
}

}  // namespace

extern "C" int asr_sr_forward_residual_dt_f32(const float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                              float* q_out, float* r_out, int batch, int n, int H, int W, int h, int w,
                                              const asr_sr_data_term* dt, asr_stream_t stream) {
    ASR_REQUIRE(x && y && rot_tf && trans_tf && q_out, "asr_sr_forward_residual_dt_f32: null pointer");
    SrDt a;
    int rc = make_data_term("asr_sr_forward_residual_dt_f32", dt, n, h, w, &a);
    if (rc != ASR_OK) return rc;
    SrDims d;
    rc = check_dims("asr_sr_forward_residual_dt_f32", batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    a.r_out = r_out;
    hipLaunchKernelGGL((sr_forward_residual_kernel<false, true>), lr_grid(d), kBlock, 0, asr_stream(stream), x, y, rot_tf,
                       trans_tf, q_out, d, a, SrMonArg<false>{});
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

namespace {

// asr_sr_config -> kernel argument; validates the host-side choices
// pd: what the caller does with ASR_OPT_PRIMAL_DUAL -- kPdUnknown (the explicit one-step entry points: the rule does not exist
// for them, they answer what they always answered to optimizer 5), kPdPriorOnly (the loss terms: only the prior is read) or
// kPdSolve (the solves: the rule's own refusals apply).
enum SrPdUse { kPdUnknown, kPdPriorOnly, kPdSolve };
int make_step(const char* fn, const asr_sr_config* cfg, bool need_update, const float* m, const float* v, const float* vhat,
              SrStep* st, SrPdUse pd = kPdUnknown) {
    ASR_REQUIRE(cfg, "%s: null config", fn);
    const int last = (pd == kPdUnknown) ? ASR_OPT_ADAMAX : ASR_OPT_PRIMAL_DUAL;
    ASR_REQUIRE(cfg->optimizer >= ASR_OPT_ADAM && cfg->optimizer <= last, "%s: unknown optimizer %d", fn, cfg->optimizer);
    ASR_REQUIRE(cfg->prior == ASR_PRIOR_TV || cfg->prior == ASR_PRIOR_BTV, "%s: unknown prior %d", fn, cfg->prior);
    if (cfg->optimizer == ASR_OPT_PRIMAL_DUAL && pd == kPdSolve) {
        ASR_UNSUPPORTED(cfg->prior == ASR_PRIOR_BTV, "%s: the primal-dual rule needs ASR_PRIOR_TV (bilateral TV has no dual form here)", fn);
        ASR_REQUIRE(cfg->c0 > 0.0f && cfg->c0 <= 0.0625f, "%s: primal-dual dual ratio c0=%g must be in (0, 1/16]", fn, (double)cfg->c0);
    }
    st->optimizer = cfg->optimizer; st->flag = cfg->flag; st->c0 = cfg->c0; st->c1 = cfg->c1; st->c2 = cfg->c2;
    st->prior = cfg->prior; st->btv_shift = 0;
    for (int k = 0; k < 9; ++k) st->btv_w[k] = 0.0f;
    if (cfg->prior == ASR_PRIOR_BTV) {
        ASR_REQUIRE(cfg->btv_shift >= 1 && cfg->btv_shift <= 4, "%s: btv_shift %d outside [1, 4]", fn, cfg->btv_shift);
        st->btv_shift = cfg->btv_shift;
        for (int k = 0; k <= 2 * cfg->btv_shift; ++k) st->btv_w[k] = powf(cfg->btv_alpha, (float)k);   // tf.pow in float32
    }
    if (need_update) {
        bool ok = true;
        switch (cfg->optimizer) {
            case ASR_OPT_ADAM: ok = m && v && (vhat || !cfg->flag); break;
            case ASR_OPT_SGD: ok = m || cfg->c0 == 0.0f; break;
            case ASR_OPT_ADAGRAD: ok = v != nullptr; break;
            default: ok = m && v; break;
        }
        ASR_REQUIRE(ok, "%s: optimizer %d needs slot buffers that were not given", fn, cfg->optimizer);
    }
    return ASR_OK;
}

asr_sr_config adam_tv_config(float one_minus_beta1, float one_minus_beta2, float epsilon, int amsgrad) {
    asr_sr_config c{};
    c.optimizer = ASR_OPT_ADAM; c.flag = amsgrad; c.c0 = one_minus_beta1; c.c1 = one_minus_beta2; c.c2 = epsilon;
    c.prior = ASR_PRIOR_TV;
    c.plane_chunk = 0;
    return c;
}

// The weights of a *_wtv entry point (nullptr, nullptr, 0, false for its *_cfg twin) -> kernel argument.  Called after
// make_step, so every refusal of the twin comes first.
struct SrTvWArg {
    const float* wy;
    const float* wx;
    int shared;
    bool weighted;
};
const SrTvWArg kNoTvW = {nullptr, nullptr, 0, false};

int make_tv_weights(const char* fn, const asr_sr_config* cfg, const SrTvWArg& a, int H, int W, SrTvW* tw) {
    tw->wy = a.wy; tw->wx = a.wx; tw->stride = a.shared ? 0 : (int64_t)H * W;
    if (!a.weighted) return ASR_OK;
    ASR_REQUIRE(a.wy && a.wx, "%s: null pointer (wy, wx)", fn);
    ASR_UNSUPPORTED(cfg->prior == ASR_PRIOR_BTV, "%s: bilateral TV has no weighted form here (edge weights need ASR_PRIOR_TV)", fn);
    return ASR_OK;
}

int sr_backward_impl(const char* fn, const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                     const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, float* grad_out,
                     int batch, int n, int H, int W, int h, int w, float lambda_df, float lambda_tv, float lambda_l2,
                     float lambda_l1, const asr_sr_config* cfg, const SrTvWArg& wa, asr_stream_t stream) {
    ASR_REQUIRE(x && resid && inv_rot_tf && inv_trans_tf, "%s: null pointer", fn);
    ASR_REQUIRE(x_new || grad_out, "%s: need x_new and/or grad_out", fn);
    ASR_REQUIRE(!x_new || alphas, "%s: alphas required with x_new", fn);
    ASR_REQUIRE(x != x_new, "%s: x_new must not alias x (the priors read neighbours)", fn);
    SrDims d;
    int rc = check_dims(fn, batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    SrStep st;
    rc = make_step(fn, cfg, x_new != nullptr, m, v, vhat, &st);
    if (rc != ASR_OK) return rc;
    SrTvW tw;
    rc = make_tv_weights(fn, cfg, wa, H, W, &tw);
    if (rc != ASR_OK) return rc;
    rc = prepare_backward(d, wa.weighted);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(sr_backward_kernel_for(d.f, wa.weighted), bwd_grid(d), kBwdBlock, bwd_lds(d), asr_stream(stream), x, x_new,
                       resid, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, grad_out, d, 2.0f * lambda_df, lambda_tv,
                       2.0f * lambda_l2, lambda_l1, st, tw);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

int sr_loss_terms_impl(const char* fn, const float* x, const float* resid, double* terms, int batch, int n, int H, int W, int h,
                       int w, const asr_sr_config* cfg, const SrTvWArg& wa, asr_stream_t stream, const SrDt* dt = nullptr) {
    // dt: resid is the RAW residual and terms[b][0] the data term's sum w * rho(r); nullptr: sum resid^2, as ever
    ASR_REQUIRE(x && resid && terms, "%s: null pointer", fn);
    ASR_REQUIRE(batch > 0 && batch <= 65535, "%s: bad batch %d", fn, batch);
    SrStep st;
    int rc = make_step(fn, cfg, false, nullptr, nullptr, nullptr, &st, kPdPriorOnly);
    if (rc != ASR_OK) return rc;
    SrTvW tw;
    rc = make_tv_weights(fn, cfg, wa, H, W, &tw);
    if (rc != ASR_OK) return rc;
    if (wa.weighted) ASR_REQUIRE(n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "%s: bad shape n=%d %dx%d <- %dx%d", fn, n, H, W, h, w);
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(terms, 0, sizeof(double) * 4 * batch, s));
    const int64_t per_image = (int64_t)n * h * w;
    if (dt) hipLaunchKernelGGL(sr_loss_df_dt_kernel, dim3(64, batch), dim3(256), 0, s, resid, terms, per_image, *dt);
    else hipLaunchKernelGGL(sr_loss_df_kernel, dim3(64, batch), dim3(256), 0, s, resid, terms, per_image);
    ASR_LAUNCH_CHECK();
    if (wa.weighted) hipLaunchKernelGGL(sr_loss_prior_kernel<true>, dim3(64, batch), dim3(256), 0, s, x, terms, H, W, st, tw);
    else hipLaunchKernelGGL(sr_loss_prior_kernel<false>, dim3(64, batch), dim3(256), 0, s, x, terms, H, W, st, tw);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

}  // namespace

extern "C" int asr_sr_backward_cfg_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                                       const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas,
                                       float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                       float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                       asr_stream_t stream) {
    return sr_backward_impl("asr_sr_backward_cfg_f32", x, x_new, resid, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, grad_out,
                            batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2, lambda_l1, cfg, kNoTvW, stream);
}

extern "C" int asr_sr_backward_wtv_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                                       const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas,
                                       float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                       float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                       const float* wy, const float* wx, int w_shared, asr_stream_t stream) {
    const SrTvWArg wa = {wy, wx, w_shared, true};
    return sr_backward_impl("asr_sr_backward_wtv_f32", x, x_new, resid, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, grad_out,
                            batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2, lambda_l1, cfg, wa, stream);
}

extern "C" int asr_sr_backward_adam_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                                        const float* inv_trans_tf, float* m, float* v, float* vhat,
                                        const float* alphas, float* grad_out, int batch, int n, int H, int W, int h,
                                        int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                                        float one_minus_beta1, float one_minus_beta2, float epsilon, int amsgrad,
                                        asr_stream_t stream) {
    const asr_sr_config c = adam_tv_config(one_minus_beta1, one_minus_beta2, epsilon, amsgrad);
    return asr_sr_backward_cfg_f32(x, x_new, resid, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, grad_out, batch, n, H, W,
                                   h, w, lambda_df, lambda_tv, lambda_l2, lambda_l1, &c, stream);
}

extern "C" int asr_sr_loss_terms_cfg_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W,
                                         int h, int w, const asr_sr_config* cfg, asr_stream_t stream) {
    return sr_loss_terms_impl("asr_sr_loss_terms_cfg_f64", x, resid, terms, batch, n, H, W, h, w, cfg, kNoTvW, stream);
}

extern "C" int asr_sr_loss_terms_wtv_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W,
                                         int h, int w, const asr_sr_config* cfg, const float* wy, const float* wx,
                                         int w_shared, asr_stream_t stream) {
    const SrTvWArg wa = {wy, wx, w_shared, true};
    return sr_loss_terms_impl("asr_sr_loss_terms_wtv_f64", x, resid, terms, batch, n, H, W, h, w, cfg, wa, stream);
}

extern "C" int asr_sr_loss_terms_dt_f64(const float* x, const float* r, double* terms, int batch, int n, int H, int W, int h,
                                        int w, const asr_sr_config* cfg, const asr_sr_data_term* dt, asr_stream_t stream) {
    SrDt a;
    const int rc = make_data_term("asr_sr_loss_terms_dt_f64", dt, n, h, w, &a);
    if (rc != ASR_OK) return rc;
    const SrTvWArg wa = {dt->wy, dt->wx, dt->tv_shared, dt->wy != nullptr};
    return sr_loss_terms_impl("asr_sr_loss_terms_dt_f64", x, r, terms, batch, n, H, W, h, w, cfg, wa, stream, &a);
}

extern "C" int asr_sr_loss_terms_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W,
                                     int h, int w, asr_stream_t stream) {
    const asr_sr_config c = adam_tv_config(0.f, 0.f, 0.f, 0);
    return asr_sr_loss_terms_cfg_f64(x, resid, terms, batch, n, H, W, h, w, &c, stream);
}

extern "C" size_t asr_sr_solve_workspace_bytes(int batch, int n, int H, int W, int h, int w) {
    return sr_workspace_bytes(batch, n, H, W, h, w, sr_plane_chunk(batch, n, H, W, 0));
}

namespace {
// ASR_OPT_PRIMAL_DUAL only: the second pair of dual planes [batch, H, W] (the Jacobi step's ping-pong), at the workspace's end
size_t sr_pd_workspace_extra(const asr_sr_config* cfg, int batch, int H, int W) {
    if (!cfg || cfg->optimizer != ASR_OPT_PRIMAL_DUAL || batch <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(float) * 2 * (size_t)batch * H * W;
}
}  // namespace

extern "C" size_t asr_sr_solve_workspace_bytes_cfg(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg) {
    return sr_workspace_bytes(batch, n, H, W, h, w, sr_plane_chunk(batch, n, H, W, cfg ? cfg->plane_chunk : 0)) +
           sr_pd_workspace_extra(cfg, batch, H, W);
}

// The whole optimisation loop of augmented_superresolution (superresolution.py:120-135) as one
// host call: num_iter x {K_fwd, K_bwd}, ping-ponging x between the caller's buffer and the
// workspace.  alphas[it*batch + b] = the per-step scalar of image b at its own global optimiser
// step (device array, prepared by the host wrapper so that the schedule and the persistent step
// counter follow optimizer.py exactly).
namespace {
// ---- convergence monitor (asr_sr_solve_mon_f32; include/asr_hip.h: the rule) ---------------------------------------
// The loss terms of the monitor, reproducible to the bit: no floating-point atomics, and every order of addition fixed by
// the image's own index space.  Image b's elements p = 0 .. P-1 (the n*h*w residuals, or the H*W pixels) are dealt to
// kMonParts workgroups of 256 threads: thread t of workgroup g adds, in float64 and in rising p, the summands of
// p = g*256 + t + k*(kMonParts*256), k = 0, 1, ...; a wave adds its 64 sums with the shuffle tree of asr_wave_sum (offsets 32,
// 16, .. 1), the workgroup its four waves as ((w0 + w1) + w2) + w3: partial g.  sr_mon_decide_kernel adds the kMonParts partials
// of a term in index order, one lane per term.  Nothing depends on the batch, on plane_chunk or on what ran before.
// The summands are those of sr_loss_df_dt_kernel and sr_loss_prior_kernel, statement for statement.
constexpr int kMonParts = 256;

__device__ __forceinline__ double sr_mon_block_sum(double acc, double* sh) {
    acc = asr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_mon_loss_df_kernel(const float* __restrict__ resid, double* __restrict__ parts,
                                                                          int64_t per_image, SrDt dt,
                                                                          const int* __restrict__ stopped) {
    __shared__ double sh[4];
    const int b = blockIdx.y;
    if (stopped[b]) return;
    const float* r = resid + (int64_t)b * per_image;
    const float* wgt = dt.w ? dt.w + (int64_t)b * dt.w_stride : nullptr;
    double acc = 0.0;
#pragma unroll 4                               // four loads in flight; the additions stay one chain, in rising p
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < per_image; p += (int64_t)kMonParts * 256) {
        const float t = r[p];
        const float a = fabsf(t);
        float rho;
        if (dt.loss == ASR_DF_L1) {
            rho = a;
        } else if (dt.loss == ASR_DF_HUBER && !(a <= dt.delta)) {
            const float lin = 2.0f * a - dt.delta;      // 2|r| is exact
            rho = dt.delta * lin;
        } else {
            rho = t * t;
        }
        if (wgt) rho = wgt[p] * rho;
        acc += (double)rho;
    }
    acc = sr_mon_block_sum(acc, sh);
    if (threadIdx.x == 0) parts[((int64_t)b * kMonParts + blockIdx.x) * 4 + 0] = acc;
}

template <bool WTV>
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_mon_loss_prior_kernel(const float* __restrict__ x, double* __restrict__ parts,
                                                                             int H, int W, SrStep st, SrTvW tw,
                                                                             const int* __restrict__ stopped) {
    __shared__ double sh[4];
    const int b = blockIdx.y;
    if (stopped[b]) return;
    const float* img = x + (int64_t)b * H * W;
    double tv = 0.0, l2 = 0.0, l1 = 0.0;
    const int64_t total = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)kMonParts * 256) {
        const int X = (int)(p % W), Y = (int)(p / W);
        const float xc = img[p];
        if (st.prior == ASR_PRIOR_BTV) {
            for (int hh = -st.btv_shift; hh <= st.btv_shift; ++hh)
                for (int vv = 0; vv <= st.btv_shift; ++vv) {
                    const int xs = X - hh, ys = Y - vv;
                    const float sv = (xs >= 0 && xs < W && ys >= 0 && ys < H) ? img[(int64_t)ys * W + xs] : 0.0f;
                    tv += (double)st.btv_w[abs(hh) + vv] * (double)fabsf(xc - sv);     // two float32 factors: exact in float64
                }
        } else if (WTV) {
            const float dy = (Y < H - 1) ? img[p + W] - xc : 0.0f;
            const float dx = (X < W - 1) ? img[p + 1] - xc : 0.0f;
            const int64_t q = (int64_t)b * tw.stride + p;      // the last row / column: weight read, times |0|
            tv += (double)(tw.wy[q] * fabsf(dy) + tw.wx[q] * fabsf(dx));
        } else {
            const float dy = (Y < H - 1) ? img[p + W] - xc : 0.0f;
            const float dx = (X < W - 1) ? img[p + 1] - xc : 0.0f;
            tv += (double)(fabsf(dy) + fabsf(dx));
        }
        l2 += (double)(xc * xc);
        l1 += (double)fabsf(xc);
    }
    tv = sr_mon_block_sum(tv, sh);
    l2 = sr_mon_block_sum(l2, sh);
    l1 = sr_mon_block_sum(l1, sh);
    if (threadIdx.x == 0) {
        double* o = parts + ((int64_t)b * kMonParts + blockIdx.x) * 4;
        o[1] = tv;
        o[2] = l2;
        o[3] = l1;
    }
}

// Per-image state of the stop rule, in the workspace.  One launch per solve.
struct SrMonState {
    double* parts;     // [batch, kMonParts, 4]
    double* best;      // [batch]
    int* stall;        // [batch]
    int* stopped;      // [batch]
};

__global__ __launch_bounds__(64) SR_NO_PK_F32 void sr_mon_init_kernel(SrMonState s, int* __restrict__ iters_done, int batch,
                                                                      int num_iter) {
    for (int b = threadIdx.x; b < batch; b += 64) {
        s.best[b] = __builtin_inf();
        s.stall[b] = 0;
        s.stopped[b] = 0;
        iters_done[b] = num_iter;
    }
}

// One evaluation.  rule == 0: only the terms (the last iteration's, for last_loss_terms, when it is no evaluation).
struct SrMonEval {
    int rule, it, row;                 // row: the evaluation's index = it / every
    int patience, min_iter;
    double rel_tol;
    double l_df, l_tv, l_l2, l_l1;     // the float32 lambdas widened
};

// One workgroup of one wave per group of `group` images (1 without coupling: per image): for each member in index order, lanes
// 0..3 add the partials of their term in index order and lane 0 forms the member's loss; the group's loss is the members'
// added in that order.  Lane 0 applies the rule to the group -- best and stall live at its first member -- and stops every
// member together (include/asr_hip.h, "multi-label coupling": the monitor).  The branches below are uniform over the workgroup.
__global__ __launch_bounds__(64) SR_NO_PK_F32 void sr_mon_decide_kernel(SrMonState s, int* __restrict__ iters_done,
                                                                        double* __restrict__ history,
                                                                        double* __restrict__ last_terms, int batch, SrMonEval e,
                                                                        int group) {
    __shared__ double t[4];
    __shared__ double part[kMonParts * 4];
    const int b0 = blockIdx.x * group;
    if (s.stopped[b0]) return;
    double loss = 0.0;
    for (int j = 0; j < group; ++j) {
        const int b = b0 + j;
        // the image's kMonParts x 4 partials through LDS (one coalesced read instead of a chain of dependent global loads)
        for (int i = threadIdx.x; i < kMonParts * 4; i += 64) part[i] = s.parts[(int64_t)b * kMonParts * 4 + i];
        __syncthreads();
        if (threadIdx.x < 4) {
            double sum = 0.0;
            for (int g = 0; g < kMonParts; ++g) sum += part[g * 4 + threadIdx.x];
            t[threadIdx.x] = sum;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (last_terms)
                for (int k = 0; k < 4; ++k) last_terms[(int64_t)b * 4 + k] = t[k];
            if (e.rule && history)
                for (int k = 0; k < 4; ++k) history[((int64_t)e.row * batch + b) * 4 + k] = t[k];
            double lb = (e.l_df * t[0] + e.l_tv * t[1]) + e.l_l2 * t[2];
            if (e.l_l1 > 0.0) lb = lb + e.l_l1 * t[3];
            loss = (j == 0) ? lb : loss + lb;
        }
        __syncthreads();                               // part and t are rewritten for the next member
    }
    if (threadIdx.x != 0 || !e.rule) return;
    const double best = s.best[b0];
    // best = +inf (no evaluation yet): the threshold is +inf itself, not inf - tol * inf = NaN; a NaN loss never improves
    const double bar = (best == __builtin_inf()) ? best : best - e.rel_tol * fabs(best);
    int stall = s.stall[b0];
    if (loss < bar) {
        s.best[b0] = loss;
        stall = 0;
    } else {
        stall += 1;
    }
    s.stall[b0] = stall;
    if (e.patience >= 1 && stall >= e.patience && e.it >= e.min_iter) {
        for (int j = 0; j < group; ++j) {
            s.stopped[b0 + j] = 1;
            iters_done[b0 + j] = e.it;
        }
    }
}

// ---- copy reweighting (include/asr_hip.h, "copy reweighting": the rule) ----------------------------------------------------------
// The four kernels and their launches (sr_rw_energy_launch, sr_rw_weights_launch, sr_rw_apply_launch, sr_rw_rearm_launch) and
// kRwMaxCopies live in sr_rw_kernels.h, a section of this translation unit.
#include "sr_rw_kernels.h"

// ---- exact adjoint (include/asr_hip.h, "exact adjoint": the rule) ------------------------------------------------------------------
// The flags kernel, the two gather kernels and their launches live in sr_adj_kernels.h, a section of this translation unit.
#include "sr_adj_kernels.h"

int check_adjoint(const char* fn, int adjoint) {
    ASR_REQUIRE(adjoint == ASR_ADJ_REGISTERED || adjoint == ASR_ADJ_EXACT, "%s: unknown adjoint %d", fn, adjoint);
    return ASR_OK;
}

int check_reweight_rule(const char* fn, int kind, double kappa) {
    ASR_REQUIRE(kind == ASR_RW_CAUCHY || kind == ASR_RW_HARD, "%s: unknown reweighting kind %d", fn, kind);
    ASR_REQUIRE(kappa > 0.0 && kappa < __builtin_inf(), "%s: reweighting kappa=%g must be finite and > 0", fn, kappa);
    return ASR_OK;
}

// The shape limits of the three launches: the ranking's LDS (n), the energy grid (batch * n), the apply grid's y (h * w)
int check_rw_shape(const char* fn, int batch, int n, int h, int w) {
    ASR_REQUIRE(batch > 0 && n > 0 && h > 0 && w > 0, "%s: bad shape batch=%d n=%d %dx%d", fn, batch, n, h, w);
    ASR_REQUIRE(n <= kRwMaxCopies, "%s: n=%d exceeds %d copies", fn, n, kRwMaxCopies);
    ASR_REQUIRE((int64_t)batch * n <= 2147483647LL, "%s: batch*n=%lld exceeds 2^31 - 1 (grid.x)", fn, (long long)batch * n);
    ASR_REQUIRE((int64_t)h * w <= 65535LL * 256, "%s: h*w=%lld exceeds %lld (grid.y)", fn, (long long)h * w, 65535LL * 256);
    return ASR_OK;
}

// Is `it` a reweighting iteration of rw, and how many lie below num_iter
bool sr_rw_is_point(const asr_sr_reweight* rw, int it) { return rw && it >= rw->start && (it - rw->start) % rw->every == 0; }
int sr_rw_points(const asr_sr_reweight* rw, int num_iter) {
    return (rw && num_iter > rw->start) ? (num_iter - rw->start + rw->every - 1) / rw->every : 0;
}
size_t sr_rw_workspace_extra(int batch, int n, int h, int w) {
    if (batch <= 0 || n <= 0 || h <= 0 || w <= 0) return 0;
    // w_eff + 8 bytes of slack to align the doubles + energy + mass
    return sizeof(float) * (size_t)batch * n * h * w + 8 + sizeof(double) * 2 * (size_t)batch * n;
}

// ---- multi-label coupling (include/asr_hip.h, "multi-label coupling") ------------------------------------------------------------
// The projection kernel lives in reduce.hip with the other per-pixel kernels over class planes (asr_simplex_project_launch,
// asr_common.h); here only the geometry of the bordered copy xb that it also writes inside a solve.
int sr_simplex_project_launch(hipStream_t s, float* x, float* xb, int groups, int G, int H, int W, const int* stopped) {
    const int64_t WP = W + 2 * kGrPadX;
    return asr_simplex_project_launch(s, x, xb, groups, G, (int64_t)H * W, W, WP, (int64_t)kGrPadY * WP + kGrPadX,
                                      (int64_t)sr_gr_plane_elems(H, W), stopped);
}

size_t sr_mon_workspace_extra(int batch) {
    // 8 bytes of slack to align the doubles + partials + best + {stall, stopped}
    return 8 + sizeof(double) * ((size_t)batch * kMonParts * 4 + (size_t)batch) + sizeof(int) * 2 * (size_t)batch;
}

int sr_solve_impl(const char* fn, float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                  const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                  double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                  float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                  const SrTvWArg& wa, asr_stream_t stream, const SrDt* dt = nullptr, const asr_sr_monitor* mon = nullptr,
                  int group = 0, const asr_sr_reweight* rw = nullptr, int adjoint = ASR_ADJ_REGISTERED) {
    // adjoint (asr_sr_solve_adj_f32; checked by the entry point): under ASR_ADJ_EXACT the flags launch is sr_adjoint_flags_kernel and
    // the gather launches are the *_adj kernels, which also read rot_tf; K_fwd, K_gt and everything else are what they were.
    // rw (asr_sr_solve_rw_f32, always with dt; checked by the entry point): on a reweighting iteration K_fwd also writes the raw
    // residual, then the three sr_rw_* launches rewrite the copy weights, w_eff (at the workspace's end) and q; from then on
    // K_fwd and the monitor's term 0 read w_eff where they read the caller's weights.  Under a monitor one more small launch
    // re-arms the stop rule.  Without rw nothing below differs from what it was.
    // group >= 1 (asr_sr_solve_ml_f32): after the update launch of an iteration's last chunk, one projection launch over the
    // batch's groups of `group` planes rewrites the new x and its bordered copy; the stop rule then decides per group.
    // mon (asr_sr_solve_mon_f32, always with dt): the MON instantiations of the three per-iteration kernels and, at every
    // evaluation, the two partial-sum kernels and the decision kernel between K_fwd and K_gt.  Everything is enqueued; the host
    // never learns during the solve which image has stopped.
    // dt (asr_sr_solve_dt_f32): K_fwd writes q = w * psi(r) where the other entry points write r; everything after reads that
    // buffer as it always did.  The workspace then ends with a second [batch*n, h, w] buffer: the raw r of the last iteration,
    // a second output of that one K_fwd launch, for the loss terms.
    ASR_REQUIRE(x && y && rot_tf && trans_tf && inv_rot_tf && inv_trans_tf && alphas && workspace, "%s: null pointer", fn);
    ASR_REQUIRE(num_iter >= 0, "%s: num_iter < 0", fn);
    SrDims d;
    int rc = check_dims(fn, batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    SrStep st;
    rc = make_step(fn, cfg, true, m, v, vhat, &st, kPdSolve);
    if (rc != ASR_OK) return rc;
    SrTvW tw;
    rc = make_tv_weights(fn, cfg, wa, H, W, &tw);
    if (rc != ASR_OK) return rc;
    const bool pd = cfg->optimizer == ASR_OPT_PRIMAL_DUAL;
    ASR_REQUIRE(group >= 0 && group <= ASR_MAX_CLASS_SET, "%s: group=%d outside 0..%d", fn, group, ASR_MAX_CLASS_SET);
    ASR_REQUIRE(group == 0 || batch % group == 0, "%s: batch=%d is no multiple of group=%d", fn, batch, group);
    ASR_UNSUPPORTED(group >= 1 && !pd, "%s: the multi-label coupling needs ASR_OPT_PRIMAL_DUAL (optimizer %d)", fn, cfg->optimizer);
    ASR_UNSUPPORTED(pd && dt && dt->loss == ASR_DF_L1, "%s: the primal-dual rule needs a smooth data term (ASR_DF_L2 or ASR_DF_HUBER)", fn);
    ASR_REQUIRE(cfg->plane_chunk >= 0, "%s: plane_chunk %d < 0", fn, cfg->plane_chunk);
    const int chunk = sr_plane_chunk(batch, n, H, W, cfg->plane_chunk);
    ASR_REQUIRE((int64_t)batch * chunk <= 65535, "%s: batch*chunk=%lld exceeds 65535 (grid.z)", fn, (long long)batch * chunk);
    const size_t base = sr_workspace_bytes(batch, n, H, W, h, w, chunk);
    const size_t pd_at = base + (dt ? sr_dt_workspace_extra(batch, n, h, w) : 0) + (mon ? sr_mon_workspace_extra(batch) : 0);
    const size_t rw_at = pd_at + sr_pd_workspace_extra(cfg, batch, H, W);
    const size_t need = rw_at + (rw ? sr_rw_workspace_extra(batch, n, h, w) : 0);
    if (workspace_bytes < need) {
        asr_set_error("%s: workspace %zu < required %zu bytes", fn, workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    hipStream_t s = asr_stream(stream);
    float* resid = static_cast<float*>(workspace);
    float* x_alt = resid + (size_t)batch * n * h * w;
    float* cur = x;
    float* nxt = x_alt;
    float* const acc = x_alt + (size_t)batch * H * W;   // running data-term sum between the chunks of an iteration
    float* const gr = acc + (size_t)batch * H * W;
    const SrGradTranslateKernel gr_kernel = sr_grad_translate_kernel_for(d.f);
    float* const xb = gr + (size_t)batch * chunk * sr_gr_plane_elems(H, W);   // bordered copy of the current x
    int* const affine_flags = reinterpret_cast<int*>(xb + (size_t)batch * sr_gr_plane_elems(H, W));
    float* const raw = reinterpret_cast<float*>(static_cast<char*>(workspace) + base);   // dt only
    SrMonState ms = {nullptr, nullptr, nullptr, nullptr};
    SrMonArg<true> marg = {nullptr};
    int mon_rows = 0;
    if (mon) {
        uintptr_t p = reinterpret_cast<uintptr_t>(raw) + sr_dt_workspace_extra(batch, n, h, w);
        p = (p + 7) & ~(uintptr_t)7;
        ms.parts = reinterpret_cast<double*>(p);
        ms.best = ms.parts + (size_t)batch * kMonParts * 4;
        ms.stall = reinterpret_cast<int*>(ms.best + batch);
        ms.stopped = ms.stall + batch;
        marg.stopped = ms.stopped;
        mon_rows = (num_iter + mon->every - 1) / mon->every;
        hipLaunchKernelGGL(sr_mon_init_kernel, dim3(1), dim3(64), 0, s, ms, mon->iters_done, batch, num_iter);
        ASR_LAUNCH_CHECK();
        if (mon->history && mon_rows > 0)     // NaN: the rows an image does not reach
            ASR_HIP_CHECK(hipMemsetAsync(mon->history, 0xFF, sizeof(double) * 4 * (size_t)mon_rows * batch, s));
    }
    // copy reweighting: w_eff, then energy and mass per copy; dtc is the data term in force (the caller's until the first reweighting)
    float* const w_eff = reinterpret_cast<float*>(static_cast<char*>(workspace) + rw_at);
    double* const rw_energy = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(w_eff + (size_t)batch * n * h * w) + 7) & ~(uintptr_t)7);
    double* const rw_mass = rw_energy + (size_t)batch * n;
    SrDt dtc = dt ? *dt : SrDt{};
    if (rw) {
        ASR_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rw->copy_weights), 0x3f800000 /* 1.0f */, (size_t)batch * n, s));
        const int points = sr_rw_points(rw, num_iter);
        if (rw->history && points > 0)        // NaN: the rows an image stopped by the monitor does not reach
            ASR_HIP_CHECK(hipMemsetAsync(rw->history, 0xFF, sizeof(float) * (size_t)points * batch * n, s));
    }
    // the three launches of a reweighting iteration, after its K_fwd (which wrote the raw residual)
    auto reweight = [&](int it, const int* stopped) -> int {
        const int per_copy = h * w;
        float* const hist = rw->history ? rw->history + (size_t)((it - rw->start) / rw->every) * batch * n : nullptr;
        int rc2 = sr_rw_energy_launch(s, raw, rw_energy, rw_mass, batch, n, per_copy, *dt, stopped);
        if (rc2 != ASR_OK) return rc2;
        rc2 = sr_rw_weights_launch(s, rw_energy, rw_mass, rw->copy_weights, hist, nullptr, batch, n, rw->kind, rw->kappa, stopped);
        if (rc2 != ASR_OK) return rc2;
        rc2 = sr_rw_apply_launch(s, raw, rw->copy_weights, w_eff, resid, batch, n, per_copy, *dt, stopped);
        if (rc2 != ASR_OK) return rc2;
        dtc.w = w_eff;
        dtc.w_stride = (int64_t)n * h * w;
        return ASR_OK;
    };
    const bool exact = adjoint == ASR_ADJ_EXACT;
    if (num_iter > 0 && exact) {
        rc = sr_adjoint_flags_launch(s, rot_tf, trans_tf, inv_rot_tf, nullptr, affine_flags, batch, n);
        if (rc != ASR_OK) return rc;
    } else if (num_iter > 0) {
        hipLaunchKernelGGL(sr_affine_flags_kernel, dim3((unsigned)batch), dim3(64), 0, s, inv_rot_tf, affine_flags, n);
        ASR_LAUNCH_CHECK();
    }
    if (num_iter > 0) {   // the borders stay zero for the whole solve; the interiors are rewritten every iteration
        const size_t pe = sr_gr_plane_elems(H, W);
        ASR_HIP_CHECK(hipMemsetAsync(gr, 0, sizeof(float) * ((size_t)batch * chunk + batch) * pe, s));
        const size_t wp = (size_t)W + 2 * kGrPadX;
        for (int b = 0; b < batch; ++b)
            ASR_HIP_CHECK(hipMemcpy2DAsync(xb + b * pe + kGrPadY * wp + kGrPadX, wp * sizeof(float), x + (size_t)b * H * W,
                                           (size_t)W * sizeof(float), (size_t)W * sizeof(float), (size_t)H,
                                           hipMemcpyDeviceToDevice, s));
    }
    // primal-dual: the duals ping-pong with x -- they sit in the caller's m (p_y) and v (p_x) whenever x sits in the caller's buffer
    float* const p_alt = reinterpret_cast<float*>(static_cast<char*>(workspace) + pd_at);
    SrPd duals = {m, v, p_alt, p_alt + (size_t)batch * H * W, cfg->c0};
    auto swap_duals = [&]() {
        if (!pd) return;
        float* const a = const_cast<float*>(duals.py);
        float* const c = const_cast<float*>(duals.px);
        duals.py = duals.py_new; duals.px = duals.px_new;
        duals.py_new = a; duals.px_new = c;
    };
    for (int it = 0; it < num_iter; ++it) {
        const bool want_terms = last_loss_terms && it == num_iter - 1;
        if (mon) {
            // an evaluation (it % every == 0) or, for last_loss_terms, the last iteration: the terms of the current x, then the rule
            const bool is_eval = it % mon->every == 0;
            const bool rw_now = sr_rw_is_point(rw, it);
            SrDt a = dtc;
            a.r_out = (is_eval || want_terms || rw_now) ? raw : nullptr;
            hipLaunchKernelGGL((sr_forward_residual_kernel<true, true, true>), lr_grid(d), kBlock, 0, s, xb, y, rot_tf, trans_tf, resid,
                               d, a, marg);
            ASR_LAUNCH_CHECK();
            if (rw_now) {
                rc = reweight(it, ms.stopped);
                if (rc != ASR_OK) return rc;
                rc = sr_rw_rearm_launch(s, ms, batch);
                if (rc != ASR_OK) return rc;
            }
            if (is_eval || want_terms) {
                hipLaunchKernelGGL(sr_mon_loss_df_kernel, dim3(kMonParts, batch), dim3(256), 0, s, raw, ms.parts,
                                   (int64_t)n * h * w, dtc, ms.stopped);
                ASR_LAUNCH_CHECK();
                if (wa.weighted)
                    hipLaunchKernelGGL(sr_mon_loss_prior_kernel<true>, dim3(kMonParts, batch), dim3(256), 0, s, cur, ms.parts, H, W, st,
                                       tw, ms.stopped);
                else
                    hipLaunchKernelGGL(sr_mon_loss_prior_kernel<false>, dim3(kMonParts, batch), dim3(256), 0, s, cur, ms.parts, H, W, st,
                                       tw, ms.stopped);
                ASR_LAUNCH_CHECK();
                SrMonEval e;
                e.rule = is_eval ? 1 : 0; e.it = it; e.row = it / mon->every;
                e.patience = mon->patience; e.min_iter = mon->min_iter; e.rel_tol = mon->rel_tol;
                e.l_df = (double)lambda_df; e.l_tv = (double)lambda_tv; e.l_l2 = (double)lambda_l2; e.l_l1 = (double)lambda_l1;
                const int members = group >= 1 ? group : 1;
                hipLaunchKernelGGL(sr_mon_decide_kernel, dim3((unsigned)(batch / members)), dim3(64), 0, s, ms, mon->iters_done,
                                   mon->history, last_loss_terms, batch, e, members);
                ASR_LAUNCH_CHECK();
            }
            const SrGradTranslateMonKernel gr_mon = sr_grad_translate_mon_kernel_for(d.f);
            for (int n0 = 0; n0 < n; n0 += chunk) {
                const int cn = n - n0 < chunk ? n - n0 : chunk;
                hipLaunchKernelGGL(gr_mon, gr_grid(d, cn), dim3(64, 4), 0, s, resid, inv_trans_tf, gr, d, 2.0f * lambda_df, n0, cn,
                                   marg);
                ASR_LAUNCH_CHECK();
                if (exact) {
                    rc = pd ? sr_gather_pd_adj_launch(s, wa.weighted, gather_grid(d), cur, nxt, gr, rot_tf, inv_rot_tf, duals,
                                                      alphas + (size_t)it * batch, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, xb, acc, n0,
                                                      cn, affine_flags, tw, marg)
                            : sr_gather_adj_launch(s, wa.weighted, gather_grid(d), cur, nxt, gr, rot_tf, inv_rot_tf, m, v, vhat,
                                                   alphas + (size_t)it * batch, nullptr, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, st,
                                                   xb, acc, n0, cn, affine_flags, tw, marg);
                    if (rc != ASR_OK) return rc;
                    continue;
                }
                if (pd) {
                    const auto pd_kernel = wa.weighted ? sr_backward_gather_pd_kernel<true, true> : sr_backward_gather_pd_kernel<false, true>;
                    hipLaunchKernelGGL(pd_kernel, gather_grid(d), dim3(64, 4), 0, s, cur, nxt, gr, inv_rot_tf, duals,
                                       alphas + (size_t)it * batch, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, xb, acc, n0, cn,
                                       affine_flags, tw, marg);
                    ASR_LAUNCH_CHECK();
                    continue;
                }
                const auto bwd_kernel = wa.weighted ? sr_backward_gather_kernel<true, true> : sr_backward_gather_kernel<false, true>;
                hipLaunchKernelGGL(bwd_kernel, gather_grid(d), dim3(64, 4), 0, s, cur, nxt, gr, inv_rot_tf, m, v, vhat,
                                   alphas + (size_t)it * batch, (float*)nullptr, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, st, xb,
                                   acc, n0, cn, affine_flags, tw, marg);
                ASR_LAUNCH_CHECK();
            }
            if (group >= 1) {
                rc = sr_simplex_project_launch(s, nxt, xb, batch / group, group, H, W, ms.stopped);
                if (rc != ASR_OK) return rc;
            }
            float* t = cur; cur = nxt; nxt = t;
            swap_duals();
            continue;
        }
        const bool rw_now = sr_rw_is_point(rw, it);
        if (dt) {
            SrDt a = dtc;
            a.r_out = (want_terms || rw_now) ? raw : nullptr;
            hipLaunchKernelGGL((sr_forward_residual_kernel<true, true>), lr_grid(d), kBlock, 0, s, xb, y, rot_tf, trans_tf, resid, d, a,
                               SrMonArg<false>{});
        } else {
            hipLaunchKernelGGL(sr_forward_residual_kernel<true>, lr_grid(d), kBlock, 0, s, xb, y, rot_tf, trans_tf, resid, d,
                               SrDtArg<false>{}, SrMonArg<false>{});
        }
        ASR_LAUNCH_CHECK();
        if (rw_now) {
            rc = reweight(it, nullptr);
            if (rc != ASR_OK) return rc;
        }
        if (want_terms) {
            rc = sr_loss_terms_impl(fn, cur, dt ? raw : resid, last_loss_terms, batch, n, H, W, h, w, cfg, wa, stream,
                                    dt ? &dtc : nullptr);
            if (rc != ASR_OK) return rc;
        }
        for (int n0 = 0; n0 < n; n0 += chunk) {
            const int cn = n - n0 < chunk ? n - n0 : chunk;
            hipLaunchKernelGGL(gr_kernel, gr_grid(d, cn), dim3(64, 4), 0, s, resid, inv_trans_tf, gr, d, 2.0f * lambda_df, n0, cn,
                               SrMonArg<false>{});
            ASR_LAUNCH_CHECK();
            if (exact) {
                rc = pd ? sr_gather_pd_adj_launch(s, wa.weighted, gather_grid(d), cur, nxt, gr, rot_tf, inv_rot_tf, duals,
                                                  alphas + (size_t)it * batch, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, xb, acc, n0, cn,
                                                  affine_flags, tw, SrMonArg<false>{})
                        : sr_gather_adj_launch(s, wa.weighted, gather_grid(d), cur, nxt, gr, rot_tf, inv_rot_tf, m, v, vhat,
                                               alphas + (size_t)it * batch, nullptr, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, st, xb,
                                               acc, n0, cn, affine_flags, tw, SrMonArg<false>{});
                if (rc != ASR_OK) return rc;
                continue;
            }
            if (pd) {
                const auto pd_kernel = wa.weighted ? sr_backward_gather_pd_kernel<true> : sr_backward_gather_pd_kernel<false>;
                hipLaunchKernelGGL(pd_kernel, gather_grid(d), dim3(64, 4), 0, s, cur, nxt, gr, inv_rot_tf, duals,
                                   alphas + (size_t)it * batch, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, xb, acc, n0, cn,
                                   affine_flags, tw, SrMonArg<false>{});
                ASR_LAUNCH_CHECK();
                continue;
            }
            const auto bwd_kernel = wa.weighted ? sr_backward_gather_kernel<true> : sr_backward_gather_kernel<false>;
            hipLaunchKernelGGL(bwd_kernel, gather_grid(d), dim3(64, 4), 0, s, cur, nxt, gr, inv_rot_tf, m, v, vhat,
                               alphas + (size_t)it * batch, (float*)nullptr, d, lambda_tv, 2.0f * lambda_l2, lambda_l1, st, xb,
                               acc, n0, cn, affine_flags, tw, SrMonArg<false>{});
            ASR_LAUNCH_CHECK();
        }
        if (group >= 1) {
            rc = sr_simplex_project_launch(s, nxt, xb, batch / group, group, H, W, nullptr);
            if (rc != ASR_OK) return rc;
        }
        float* t = cur; cur = nxt; nxt = t;
        swap_duals();
    }
    if (cur != x) {
        const size_t bytes = sizeof(float) * (size_t)batch * H * W;
        ASR_HIP_CHECK(hipMemcpyAsync(x, cur, bytes, hipMemcpyDeviceToDevice, s));
        if (pd) {    // the duals moved with x: back into the caller's slots
            ASR_HIP_CHECK(hipMemcpyAsync(m, duals.py, bytes, hipMemcpyDeviceToDevice, s));
            ASR_HIP_CHECK(hipMemcpyAsync(v, duals.px, bytes, hipMemcpyDeviceToDevice, s));
        }
    }
    return ASR_OK;
}

// wy[Y,X] = 1 / (1 + beta * |I[Y+1,X] - I[Y,X]|^2), wx the same along X; the last row of wy and the last column of wx are 1
// (include/asr_hip.h: the rule).  One thread per pixel; every product and sum rounds by itself, in the order written.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_tv_edge_weights_kernel(const float* __restrict__ guide, float* __restrict__ wy,
                                                                              float* __restrict__ wx, int H, int W, float beta) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    if (X >= W || Y >= H) return;
    const int64_t o = ((int64_t)blockIdx.z * H + Y) * W + X;
    // (no lambda: one would not inherit the kernel's target attribute and would stay a call with its captures in scratch)
    const float* c = guide + o * 3;
    const float c0 = c[0], c1 = c[1], c2 = c[2];
    float vy = 1.0f, vx = 1.0f;
    if (Y < H - 1) {
        const float* q = c + (int64_t)W * 3;
        const float a0 = q[0] - c0, a1 = q[1] - c1, a2 = q[2] - c2;
        const float dd = (a0 * a0 + a1 * a1) + a2 * a2;
        vy = 1.0f / (1.0f + beta * dd);
    }
    if (X < W - 1) {
        const float a0 = c[3] - c0, a1 = c[4] - c1, a2 = c[5] - c2;
        const float dd = (a0 * a0 + a1 * a1) + a2 * a2;
        vx = 1.0f / (1.0f + beta * dd);
    }
    wy[o] = vy;
    wx[o] = vx;
}
}  // namespace

extern "C" int asr_tv_edge_weights_f32(const float* guide, float* wy, float* wx, int batch, int H, int W, float beta,
                                       asr_stream_t stream) {
    ASR_REQUIRE(guide && wy && wx, "asr_tv_edge_weights_f32: null pointer");
    ASR_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0, "asr_tv_edge_weights_f32: bad shape batch=%d %dx%d", batch, H, W);
    ASR_REQUIRE(beta >= 0.0f && beta < __builtin_inff(), "asr_tv_edge_weights_f32: beta=%g must be finite and >= 0", (double)beta);
    SrDims d;
    d.batch = batch; d.n = 1; d.H = H; d.W = W; d.h = H; d.w = W; d.f = 0;
    hipLaunchKernelGGL(sr_tv_edge_weights_kernel, hr_grid(d), kBlock, 0, asr_stream(stream), guide, wy, wx, H, W, beta);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_sr_solve_cfg_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                    const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                    const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                    size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                                    float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                                    const asr_sr_config* cfg, asr_stream_t stream) {
    return sr_solve_impl("asr_sr_solve_cfg_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                         last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                         lambda_l1, cfg, kNoTvW, stream);
}

extern "C" int asr_sr_solve_wtv_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                    const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                    const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                    size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                                    float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                                    const asr_sr_config* cfg, const float* wy, const float* wx, int w_shared,
                                    asr_stream_t stream) {
    const SrTvWArg wa = {wy, wx, w_shared, true};
    return sr_solve_impl("asr_sr_solve_wtv_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                         last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                         lambda_l1, cfg, wa, stream);
}

extern "C" size_t asr_sr_solve_workspace_bytes_dt(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg) {
    return asr_sr_solve_workspace_bytes_cfg(batch, n, H, W, h, w, cfg) + sr_dt_workspace_extra(batch, n, h, w);
}

namespace {
// asr_sr_solve_dt_f32 (mon NULL) and asr_sr_solve_mon_f32 (mon given, checked here), with the group of asr_sr_solve_ml_f32
int sr_solve_dt_entry(const char* fn, float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                      const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                      double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                      float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                      const asr_sr_data_term* dt, const asr_sr_monitor* mon, bool monitored, int group, asr_stream_t stream,
                      const asr_sr_reweight* rw = nullptr, int adjoint = ASR_ADJ_REGISTERED) {
    int rc = check_adjoint(fn, adjoint);
    if (rc != ASR_OK) return rc;
    SrDt a;
    rc = make_data_term(fn, dt, n, h, w, &a);
    if (rc != ASR_OK) return rc;
    if (rw) {
        rc = check_reweight_rule(fn, rw->kind, rw->kappa);
        if (rc != ASR_OK) return rc;
        ASR_REQUIRE(rw->every >= 1, "%s: reweighting every=%d must be >= 1", fn, rw->every);
        ASR_REQUIRE(rw->start >= 0, "%s: reweighting start=%d must be >= 0", fn, rw->start);
        ASR_REQUIRE(rw->copy_weights, "%s: null pointer (reweighting copy_weights)", fn);
        rc = check_rw_shape(fn, batch, n, h, w);          // n <= 640 and the grid limits of the three launches, as stand-alone
        if (rc != ASR_OK) return rc;
    }
    if (monitored) {
        ASR_REQUIRE(mon, "%s: null monitor", fn);
        ASR_REQUIRE(mon->every >= 1, "%s: monitor every=%d must be >= 1", fn, mon->every);
        ASR_REQUIRE(mon->rel_tol >= 0.0 && mon->rel_tol < __builtin_inf(), "%s: monitor rel_tol=%g must be finite and >= 0", fn,
                    mon->rel_tol);
        ASR_REQUIRE(mon->patience >= 0, "%s: monitor patience=%d must be >= 0", fn, mon->patience);
        ASR_REQUIRE(mon->min_iter >= 0, "%s: monitor min_iter=%d must be >= 0", fn, mon->min_iter);
        ASR_REQUIRE(mon->iters_done, "%s: null pointer (monitor iters_done)", fn);
    }
    const SrTvWArg wa = {dt->wy, dt->wx, dt->tv_shared, dt->wy != nullptr};
    return sr_solve_impl(fn, x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter, last_loss_terms,
                         workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2, lambda_l1, cfg, wa,
                         stream, &a, monitored ? mon : nullptr, group, rw, adjoint);
}
}  // namespace

extern "C" int asr_sr_solve_dt_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                   const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                   const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                   size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                   float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                   const asr_sr_data_term* dt, asr_stream_t stream) {
    return sr_solve_dt_entry("asr_sr_solve_dt_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                             last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                             lambda_l1, cfg, dt, nullptr, false, 0, stream);
}

extern "C" size_t asr_sr_solve_workspace_bytes_mon(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg) {
    return asr_sr_solve_workspace_bytes_dt(batch, n, H, W, h, w, cfg) + sr_mon_workspace_extra(batch > 0 ? batch : 0);
}

extern "C" int asr_sr_solve_mon_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                    const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                    const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                    size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                    float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                    const asr_sr_data_term* dt, const asr_sr_monitor* mon, asr_stream_t stream) {
    return sr_solve_dt_entry("asr_sr_solve_mon_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                             last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                             lambda_l1, cfg, dt, mon, true, 0, stream);
}

// ---- multi-label coupling: the entry points (include/asr_hip.h, "multi-label coupling") ---------------------------------------------
extern "C" int asr_simplex_project_f32(float* x, int groups, int group, int64_t pixels, asr_stream_t stream) {
    ASR_REQUIRE(x, "asr_simplex_project_f32: null pointer");
    ASR_REQUIRE(group >= 1 && group <= ASR_MAX_CLASS_SET, "asr_simplex_project_f32: group=%d outside 1..%d", group, ASR_MAX_CLASS_SET);
    ASR_REQUIRE(groups >= 1 && pixels >= 1, "asr_simplex_project_f32: bad shape groups=%d pixels=%lld", groups, (long long)pixels);
    return asr_simplex_project_launch(asr_stream(stream), x, nullptr, groups, group, pixels, 1, 0, 0, 0, nullptr);
}

extern "C" size_t asr_sr_solve_workspace_bytes_ml(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg,
                                                  int monitored) {
    return monitored ? asr_sr_solve_workspace_bytes_mon(batch, n, H, W, h, w, cfg)
                     : asr_sr_solve_workspace_bytes_dt(batch, n, H, W, h, w, cfg);
}

extern "C" int asr_sr_solve_ml_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                   const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                   const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                   size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                   float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                   const asr_sr_data_term* dt, const asr_sr_monitor* mon, int group, asr_stream_t stream) {
    return sr_solve_dt_entry("asr_sr_solve_ml_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                             last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                             lambda_l1, cfg, dt, mon, mon != nullptr, group, stream);
}

// ---- copy reweighting: the entry points (include/asr_hip.h, "copy reweighting") --------------------------------------------------
extern "C" int asr_sr_copy_energy_f64(const float* r, const asr_sr_data_term* dt, double* energy, double* mass, int batch, int n,
                                      int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(r && energy && mass, "asr_sr_copy_energy_f64: null pointer");
    SrDt a;
    int rc = make_data_term("asr_sr_copy_energy_f64", dt, n, h, w, &a);
    if (rc != ASR_OK) return rc;
    rc = check_rw_shape("asr_sr_copy_energy_f64", batch, n, h, w);
    if (rc != ASR_OK) return rc;
    return sr_rw_energy_launch(asr_stream(stream), r, energy, mass, batch, n, h * w, a, nullptr);
}

extern "C" int asr_sr_copy_weights_f32(const double* energy, const double* mass, int kind, double kappa, float* c, double* scale_out,
                                       int batch, int n, asr_stream_t stream) {
    ASR_REQUIRE(energy && mass && c, "asr_sr_copy_weights_f32: null pointer");
    int rc = check_reweight_rule("asr_sr_copy_weights_f32", kind, kappa);
    if (rc != ASR_OK) return rc;
    rc = check_rw_shape("asr_sr_copy_weights_f32", batch, n, 1, 1);
    if (rc != ASR_OK) return rc;
    return sr_rw_weights_launch(asr_stream(stream), energy, mass, c, nullptr, scale_out, batch, n, kind, kappa, nullptr);
}

extern "C" int asr_sr_apply_copy_weights_f32(const float* r, const asr_sr_data_term* dt, const float* c, float* w_eff, float* q,
                                             int batch, int n, int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(r && c && w_eff && q, "asr_sr_apply_copy_weights_f32: null pointer");
    SrDt a;
    int rc = make_data_term("asr_sr_apply_copy_weights_f32", dt, n, h, w, &a);
    if (rc != ASR_OK) return rc;
    rc = check_rw_shape("asr_sr_apply_copy_weights_f32", batch, n, h, w);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(w_eff != a.w, "asr_sr_apply_copy_weights_f32: w_eff aliases the data term's weights");
    return sr_rw_apply_launch(asr_stream(stream), r, c, w_eff, q, batch, n, h * w, a, nullptr);
}

extern "C" size_t asr_sr_solve_workspace_bytes_rw(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg,
                                                  int monitored) {
    return asr_sr_solve_workspace_bytes_ml(batch, n, H, W, h, w, cfg, monitored) + sr_rw_workspace_extra(batch, n, h, w);
}

extern "C" int asr_sr_solve_rw_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                   const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                   const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                   size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                   float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                   const asr_sr_data_term* dt, const asr_sr_monitor* mon, int group,
                                   const asr_sr_reweight* rw, asr_stream_t stream) {
    return sr_solve_dt_entry("asr_sr_solve_rw_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                             last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                             lambda_l1, cfg, dt, mon, mon != nullptr, group, stream, rw);
}

// ---- exact adjoint: the entry points (include/asr_hip.h, "exact adjoint") ---------------------------------------------------------
extern "C" int asr_sr_solve_adj_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                    const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                    const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                    size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                                    float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                    const asr_sr_data_term* dt, const asr_sr_monitor* mon, int group,
                                    const asr_sr_reweight* rw, int adjoint, asr_stream_t stream) {
    return sr_solve_dt_entry("asr_sr_solve_adj_f32", x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                             last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv, lambda_l2,
                             lambda_l1, cfg, dt, mon, mon != nullptr, group, stream, rw, adjoint);
}

extern "C" int asr_sr_adjoint_flags_i32(const float* rot_tf, const float* trans_tf, const float* inv_rot_tf, int* flags, int batch,
                                        int n, asr_stream_t stream) {
    ASR_REQUIRE(rot_tf && trans_tf && inv_rot_tf && flags, "asr_sr_adjoint_flags_i32: null pointer");
    ASR_REQUIRE(batch > 0 && n > 0, "asr_sr_adjoint_flags_i32: bad shape batch=%d n=%d", batch, n);
    return sr_adjoint_flags_launch(asr_stream(stream), rot_tf, trans_tf, inv_rot_tf, flags, nullptr, batch, n);
}

namespace {
// the running data-term sum [batch, H, W] + the G_R planes of a chunk + one mode word per image
size_t sr_backward_adj_bytes(int batch, int H, int W, int chunk) {
    return sizeof(float) * ((size_t)batch * H * W + (size_t)batch * chunk * sr_gr_plane_elems(H, W)) + sizeof(int) * (size_t)batch;
}
}  // namespace

extern "C" size_t asr_sr_backward_adj_workspace_bytes(int batch, int n, int H, int W, const asr_sr_config* cfg) {
    if (batch <= 0 || n <= 0 || H <= 0 || W <= 0) return 0;
    return sr_backward_adj_bytes(batch, H, W, sr_plane_chunk(batch, n, H, W, cfg ? cfg->plane_chunk : 0));
}

extern "C" int asr_sr_backward_adj_f32(const float* x, float* x_new, const float* resid, const float* rot_tf, const float* trans_tf,
                                       const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                       const float* alphas, float* grad_out, int batch, int n, int H, int W, int h, int w,
                                       float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                                       const float* wy, const float* wx, int w_shared, int adjoint, void* workspace,
                                       size_t workspace_bytes, asr_stream_t stream) {
    const char* fn = "asr_sr_backward_adj_f32";
    int rc = check_adjoint(fn, adjoint);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE((wy == nullptr) == (wx == nullptr), "%s: null pointer (wy, wx: both or neither)", fn);
    const SrTvWArg wa = {wy, wx, w_shared, wy != nullptr};
    if (adjoint == ASR_ADJ_REGISTERED)      // the fused one-launch kernel of asr_sr_backward_wtv_f32 / _cfg_f32; no workspace
        return sr_backward_impl(fn, x, x_new, resid, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, grad_out, batch, n, H, W, h, w,
                                lambda_df, lambda_tv, lambda_l2, lambda_l1, cfg, wa, stream);
    ASR_REQUIRE(x && resid && rot_tf && trans_tf && inv_rot_tf && inv_trans_tf && workspace, "%s: null pointer", fn);
    ASR_REQUIRE(x_new || grad_out, "%s: need x_new and/or grad_out", fn);
    ASR_REQUIRE(!x_new || alphas, "%s: alphas required with x_new", fn);
    ASR_REQUIRE(x != x_new, "%s: x_new must not alias x (the priors read neighbours)", fn);
    SrDims d;
    rc = check_dims(fn, batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    SrStep st;
    rc = make_step(fn, cfg, x_new != nullptr, m, v, vhat, &st);
    if (rc != ASR_OK) return rc;
    SrTvW tw;
    rc = make_tv_weights(fn, cfg, wa, H, W, &tw);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(cfg->plane_chunk >= 0, "%s: plane_chunk %d < 0", fn, cfg->plane_chunk);
    const int chunk = sr_plane_chunk(batch, n, H, W, cfg->plane_chunk);
    ASR_REQUIRE((int64_t)batch * chunk <= 65535, "%s: batch*chunk=%lld exceeds 65535 (grid.z)", fn, (long long)batch * chunk);
    const size_t need = sr_backward_adj_bytes(batch, H, W, chunk);
    if (workspace_bytes < need) {
        asr_set_error("%s: workspace %zu < required %zu bytes", fn, workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    hipStream_t s = asr_stream(stream);
    float* const acc = static_cast<float*>(workspace);
    float* const gr = acc + (size_t)batch * H * W;
    int* const mode = reinterpret_cast<int*>(gr + (size_t)batch * chunk * sr_gr_plane_elems(H, W));
    ASR_HIP_CHECK(hipMemsetAsync(gr, 0, sizeof(float) * (size_t)batch * chunk * sr_gr_plane_elems(H, W), s));   // the borders
    rc = sr_adjoint_flags_launch(s, rot_tf, trans_tf, inv_rot_tf, nullptr, mode, batch, n);
    if (rc != ASR_OK) return rc;
    const SrGradTranslateKernel gr_kernel = sr_grad_translate_kernel_for(d.f);
    for (int n0 = 0; n0 < n; n0 += chunk) {
        const int cn = n - n0 < chunk ? n - n0 : chunk;
        hipLaunchKernelGGL(gr_kernel, gr_grid(d, cn), dim3(64, 4), 0, s, resid, inv_trans_tf, gr, d, 2.0f * lambda_df, n0, cn,
                           SrMonArg<false>{});
        ASR_LAUNCH_CHECK();
        rc = sr_gather_adj_launch(s, wa.weighted, gather_grid(d), x, x_new, gr, rot_tf, inv_rot_tf, m, v, vhat, alphas, grad_out, d,
                                  lambda_tv, 2.0f * lambda_l2, lambda_l1, st, nullptr, acc, n0, cn, mode, tw, SrMonArg<false>{});
        if (rc != ASR_OK) return rc;
    }
    return ASR_OK;
}

// ---- the step bound of the primal-dual rule (asr_sr_data_bound_f32; include/asr_hip.h, "primal-dual": the rule) -------------
// One repetition is one solver iteration on v with measurements of zero -- K_fwd, K_gt and the gather kernel as they are, the
// gather's gradient output (no prior: every lambda but lambda_df is 0) taken as w = M v -- then the two maxima and v = w / s.
namespace {
constexpr int kBoundMaxIters = 64, kBoundParts = 64;

// maxima[b] = {max over v > 0 of w / v, max w} as the bits of floats >= 0 (their order as unsigned integers is their order as
// floats), zeroed before the launch: integer maxima, the same bits in any order of arrival.
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_bound_maxima_kernel(const float* __restrict__ wv, const float* __restrict__ v,
                                                                           unsigned* __restrict__ maxima, int64_t per_image) {
    const int b = blockIdx.y;
    const float* wp = wv + (int64_t)b * per_image;
    const float* vp = v + (int64_t)b * per_image;
    float ratio = 0.0f, top = 0.0f;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < per_image; p += (int64_t)kBoundParts * 256) {
        const float wi = wp[p], vi = vp[p];
        if (vi > 0.0f) ratio = fmaxf(ratio, wi / vi);
        top = fmaxf(top, wi);
    }
    ratio = asr_wave_max(ratio);
    top = asr_wave_max(top);
    if ((threadIdx.x & 63) == 0) {
        if (ratio > 0.0f) atomicMax(maxima + (int64_t)b * 2 + 0, __float_as_uint(ratio));
        if (top > 0.0f) atomicMax(maxima + (int64_t)b * 2 + 1, __float_as_uint(top));
    }
}

// v for the next repetition, plain and zero-bordered: 1 everywhere to begin with (maxima == nullptr), then w / s while s > 0
// (s == 0: w is 0 everywhere, v stays and every later repetition finds the same maxima, the bound of the last one done)
__global__ __launch_bounds__(256) SR_NO_PK_F32 void sr_bound_next_v_kernel(const float* __restrict__ wv, float* __restrict__ v,
                                                                           float* __restrict__ v_bordered,
                                                                           const unsigned* __restrict__ maxima, int H, int W) {
    const int X = blockIdx.x * kTileX + threadIdx.x;
    const int Y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (X >= W || Y >= H) return;
    const int64_t o = ((int64_t)b * H + Y) * W + X;
    float nv = 1.0f;
    if (maxima) {
        const float s = __uint_as_float(maxima[(int64_t)b * 2 + 1]);
        if (!(s > 0.0f)) return;
        nv = wv[o] / s;
    }
    v[o] = nv;
    v_bordered[(size_t)b * sr_gr_plane_elems(H, W) + (size_t)(Y + kGrPadY) * (W + 2 * kGrPadX) + (X + kGrPadX)] = nv;
}

__global__ __launch_bounds__(64) void sr_bound_out_kernel(const unsigned* __restrict__ maxima, float* __restrict__ bound, int batch) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < batch) bound[b] = __uint_as_float(maxima[(int64_t)b * 2]);
}

// measurements of zero + residuals + v, w, the running sum + the planes of a chunk and of v + the affine flags + the maxima
size_t sr_bound_workspace_bytes(int batch, int n, int H, int W, int h, int w, int chunk) {
    return sizeof(float) * (2 * (size_t)batch * n * h * w + 3 * (size_t)batch * H * W +
                            ((size_t)batch * chunk + batch) * sr_gr_plane_elems(H, W)) +
           sizeof(int) * (size_t)batch + sizeof(unsigned) * 2 * (size_t)kBoundMaxIters * batch;
}
}  // namespace

extern "C" size_t asr_sr_data_bound_workspace_bytes(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg) {
    if (batch <= 0 || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return 0;
    return sr_bound_workspace_bytes(batch, n, H, W, h, w, sr_plane_chunk(batch, n, H, W, cfg ? cfg->plane_chunk : 0));
}

namespace {
int sr_data_bound_impl(const char* fn, float* bound, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                       const float* inv_trans_tf, const float* weights, int weights_shared, int iters, void* workspace,
                       size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df, const asr_sr_config* cfg,
                       int adjoint, asr_stream_t stream) {
    ASR_REQUIRE(bound && rot_tf && trans_tf && inv_rot_tf && inv_trans_tf && workspace, "%s: null pointer", fn);
    ASR_REQUIRE(iters >= 1 && iters <= kBoundMaxIters, "%s: iters=%d outside [1, %d]", fn, iters, kBoundMaxIters);
    ASR_REQUIRE(lambda_df >= 0.0f && lambda_df < __builtin_inff(), "%s: lambda_df=%g must be finite and >= 0", fn, (double)lambda_df);
    SrDims d;
    int rc = check_dims(fn, batch, n, H, W, h, w, &d);
    if (rc != ASR_OK) return rc;
    const int requested = cfg ? cfg->plane_chunk : 0;
    ASR_REQUIRE(requested >= 0, "%s: plane_chunk %d < 0", fn, requested);
    const int chunk = sr_plane_chunk(batch, n, H, W, requested);
    ASR_REQUIRE((int64_t)batch * chunk <= 65535, "%s: batch*chunk=%lld exceeds 65535 (grid.z)", fn, (long long)batch * chunk);
    const size_t need = sr_bound_workspace_bytes(batch, n, H, W, h, w, chunk);
    if (workspace_bytes < need) {
        asr_set_error("%s: workspace %zu < required %zu bytes", fn, workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    hipStream_t s = asr_stream(stream);
    const size_t lr = (size_t)batch * n * h * w, hr = (size_t)batch * H * W, pe = sr_gr_plane_elems(H, W);
    float* const zero_y = static_cast<float*>(workspace);
    float* const resid = zero_y + lr;
    float* const vcur = resid + lr;
    float* const wv = vcur + hr;
    float* const acc = wv + hr;
    float* const gr = acc + hr;
    float* const vb = gr + (size_t)batch * chunk * pe;
    int* const affine_flags = reinterpret_cast<int*>(vb + (size_t)batch * pe);
    unsigned* const maxima = reinterpret_cast<unsigned*>(affine_flags + batch);
    ASR_HIP_CHECK(hipMemsetAsync(zero_y, 0, sizeof(float) * lr, s));
    ASR_HIP_CHECK(hipMemsetAsync(gr, 0, sizeof(float) * ((size_t)batch * chunk + batch) * pe, s));
    ASR_HIP_CHECK(hipMemsetAsync(maxima, 0, sizeof(unsigned) * 2 * (size_t)iters * batch, s));
    const bool exact = adjoint == ASR_ADJ_EXACT;
    if (exact) {
        rc = sr_adjoint_flags_launch(s, rot_tf, trans_tf, inv_rot_tf, nullptr, affine_flags, batch, n);
        if (rc != ASR_OK) return rc;
    } else {
        hipLaunchKernelGGL(sr_affine_flags_kernel, dim3((unsigned)batch), dim3(64), 0, s, inv_rot_tf, affine_flags, n);
        ASR_LAUNCH_CHECK();
    }
    SrDt dt;
    dt.loss = ASR_DF_L2; dt.delta = 0.0f; dt.w = weights; dt.w_stride = weights_shared ? 0 : (int64_t)n * h * w; dt.r_out = nullptr;
    SrStep st = {};
    st.optimizer = ASR_OPT_ADAM; st.prior = ASR_PRIOR_TV;
    const SrTvW tw = {nullptr, nullptr, 0};
    const SrGradTranslateKernel gr_kernel = sr_grad_translate_kernel_for(d.f);
    for (int k = 0; k < iters; ++k) {
        unsigned* const mk = maxima + (size_t)k * 2 * batch;
        hipLaunchKernelGGL(sr_bound_next_v_kernel, hr_grid(d), kBlock, 0, s, wv, vcur, vb, k ? mk - 2 * batch : nullptr, H, W);
        ASR_LAUNCH_CHECK();
        hipLaunchKernelGGL((sr_forward_residual_kernel<true, true>), lr_grid(d), kBlock, 0, s, vb, zero_y, rot_tf, trans_tf, resid, d, dt,
                           SrMonArg<false>{});
        ASR_LAUNCH_CHECK();
        for (int n0 = 0; n0 < n; n0 += chunk) {
            const int cn = n - n0 < chunk ? n - n0 : chunk;
            hipLaunchKernelGGL(gr_kernel, gr_grid(d, cn), dim3(64, 4), 0, s, resid, inv_trans_tf, gr, d, 2.0f * lambda_df, n0, cn,
                               SrMonArg<false>{});
            ASR_LAUNCH_CHECK();
            if (exact) {
                rc = sr_gather_adj_launch(s, false, gather_grid(d), vcur, nullptr, gr, rot_tf, inv_rot_tf, nullptr, nullptr, nullptr,
                                          nullptr, wv, d, 0.0f, 0.0f, 0.0f, st, nullptr, acc, n0, cn, affine_flags, tw, SrMonArg<false>{});
                if (rc != ASR_OK) return rc;
                continue;
            }
            hipLaunchKernelGGL(sr_backward_gather_kernel<false>, gather_grid(d), dim3(64, 4), 0, s, vcur, (float*)nullptr, gr, inv_rot_tf,
                               (float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, wv, d, 0.0f, 0.0f, 0.0f, st,
                               (float*)nullptr, acc, n0, cn, affine_flags, tw, SrMonArg<false>{});
            ASR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sr_bound_maxima_kernel, dim3(kBoundParts, batch), dim3(256), 0, s, wv, vcur, mk, (int64_t)H * W);
        ASR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sr_bound_out_kernel, dim3((unsigned)asr_cdiv(batch, 64)), dim3(64), 0, s, maxima + (size_t)(iters - 1) * 2 * batch,
                       bound, batch);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
}  // namespace

extern "C" int asr_sr_data_bound_f32(float* bound, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                                     const float* inv_trans_tf, const float* weights, int weights_shared, int iters,
                                     void* workspace, size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                                     float lambda_df, const asr_sr_config* cfg, asr_stream_t stream) {
    return sr_data_bound_impl("asr_sr_data_bound_f32", bound, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, weights, weights_shared, iters,
                              workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, cfg, ASR_ADJ_REGISTERED, stream);
}

extern "C" int asr_sr_data_bound_adj_f32(float* bound, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                                         const float* inv_trans_tf, const float* weights, int weights_shared, int iters,
                                         void* workspace, size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                                         float lambda_df, const asr_sr_config* cfg, int adjoint, asr_stream_t stream) {
    const int rc = check_adjoint("asr_sr_data_bound_adj_f32", adjoint);
    if (rc != ASR_OK) return rc;
    return sr_data_bound_impl("asr_sr_data_bound_adj_f32", bound, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, weights, weights_shared,
                              iters, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, cfg, adjoint, stream);
}

extern "C" int asr_sr_solve_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                                const float* alphas, int num_iter, double* last_loss_terms, void* workspace,
                                size_t workspace_bytes, int batch, int n, int H, int W, int h, int w,
                                float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                                float one_minus_beta1, float one_minus_beta2, float epsilon, int amsgrad,
                                asr_stream_t stream) {
    const asr_sr_config c = adam_tv_config(one_minus_beta1, one_minus_beta2, epsilon, amsgrad);
    return asr_sr_solve_cfg_f32(x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, m, v, vhat, alphas, num_iter,
                                last_loss_terms, workspace, workspace_bytes, batch, n, H, W, h, w, lambda_df, lambda_tv,
                                lambda_l2, lambda_l1, &c, stream);
}

static int realign_common(int mode, const float* y, float* out_a, float* out_b, const float* trans_tf, const float* rot_tf,
                          int batch, int n, int H, int W, int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(y && out_a && trans_tf && rot_tf && (mode != 2 || out_b), "asr_realign: null pointer");
    ASR_REQUIRE(batch > 0 && batch <= 65535 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "asr_realign: bad shape");
    SrDims d;
    d.batch = batch; d.n = n; d.H = H; d.W = W; d.h = h; d.w = w; d.f = 0;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipStream_t s = asr_stream(stream);
    if (mode == 1) hipLaunchKernelGGL(sr_realign_kernel<1>, hr_grid(d), kBlock, 0, s, y, out_a, out_b, trans_tf, rot_tf, d, sy, sx);
    else if (mode == 0) hipLaunchKernelGGL(sr_realign_kernel<0>, hr_grid(d), kBlock, 0, s, y, out_a, out_b, trans_tf, rot_tf, d, sy, sx);
    else hipLaunchKernelGGL(sr_realign_kernel<2>, hr_grid(d), kBlock, 0, s, y, out_a, out_b, trans_tf, rot_tf, d, sy, sx);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_realign_max_f32(const float* y, float* out, const float* trans_tf, const float* rot_tf, int batch,
                                   int n, int H, int W, int h, int w, asr_stream_t stream) {
    return realign_common(1, y, out, nullptr, trans_tf, rot_tf, batch, n, H, W, h, w, stream);
}

extern "C" int asr_realign_mean_f32(const float* y, float* out, const float* trans_tf, const float* rot_tf, int batch,
                                    int n, int H, int W, int h, int w, asr_stream_t stream) {
    return realign_common(0, y, out, nullptr, trans_tf, rot_tf, batch, n, H, W, h, w, stream);
}

extern "C" int asr_realign_max_mean_f32(const float* y, float* out_max, float* out_mean, const float* trans_tf,
                                        const float* rot_tf, int batch, int n, int H, int W, int h, int w,
                                        asr_stream_t stream) {
    return realign_common(2, y, out_max, out_mean, trans_tf, rot_tf, batch, n, H, W, h, w, stream);
}

extern "C" int asr_realign_select_max_copies(void) { return kSelMaxCopies; }

extern "C" int asr_realign_select_f32(const float* y, float* out_q, float* out_trim, const int* lo_rank, const int* hi_rank,
                                      const float* t, int num_q, int trim_k, const float* trans_tf, const float* rot_tf,
                                      int batch, int n, int H, int W, int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(y && trans_tf && rot_tf, "asr_realign_select_f32: null pointer");
    ASR_REQUIRE(num_q >= 0 && num_q <= kSelMaxQ, "asr_realign_select_f32: num_q=%d (0..%d)", num_q, kSelMaxQ);
    ASR_REQUIRE(num_q > 0 || out_trim, "asr_realign_select_f32: nothing to compute (num_q = 0 and no out_trim)");
    ASR_REQUIRE(num_q == 0 || (out_q && lo_rank && hi_rank && t), "asr_realign_select_f32: null pointer");
    ASR_REQUIRE(batch > 0 && batch <= 65535 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "asr_realign_select_f32: bad shape");
    ASR_UNSUPPORTED(n > kSelMaxCopies, "asr_realign_select_f32: n=%d copies, at most %d (256 bytes of LDS per copy, 160 KiB per workgroup)",
                    n, kSelMaxCopies);
    SrSelect sel = {};
    sel.num_q = num_q;
    for (int j = 0; j < num_q; ++j) {
        ASR_REQUIRE(lo_rank[j] >= 0 && lo_rank[j] <= hi_rank[j] && hi_rank[j] <= n - 1,
                    "asr_realign_select_f32: ranks[%d] = (%d, %d) need 0 <= lo <= hi <= n - 1 = %d", j, lo_rank[j], hi_rank[j], n - 1);
        sel.lo[j] = lo_rank[j]; sel.hi[j] = hi_rank[j]; sel.t[j] = t[j];
    }
    ASR_REQUIRE(trim_k >= 0 && 2 * (int64_t)trim_k < n, "asr_realign_select_f32: trim_k=%d needs 0 <= 2k < n = %d", trim_k, n);
    ASR_REQUIRE(out_trim || trim_k == 0, "asr_realign_select_f32: trim_k=%d without out_trim", trim_k);
    sel.trim_k = trim_k;
    const int64_t tiles_x = asr_cdiv(W, kSelX), tiles = tiles_x * asr_cdiv(H, kSelY);
    ASR_REQUIRE(tiles <= 0x7fffffff, "asr_realign_select_f32: %dx%d output exceeds the grid", H, W);
    SrDims d;
    d.batch = batch; d.n = n; d.H = H; d.W = W; d.h = h; d.w = w; d.f = 0;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const size_t lds = sizeof(unsigned) * (size_t)n * kSelPix;
    static AsrDeviceOnce once;
    if (lds > 64 * 1024)
        ASR_HIP_CHECK(asr_allow_dynamic_lds(once, reinterpret_cast<const void*>(sr_realign_select_kernel), kSelLdsMax));
    hipLaunchKernelGGL(sr_realign_select_kernel, dim3((unsigned)tiles, 1, (unsigned)batch), dim3(kSelX, kSelY), lds,
                       asr_stream(stream), y, out_q, out_trim, trans_tf, rot_tf, d, sel, (int)tiles_x, sy, sx);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_realign_covered_f32(const float* y, const float* wgt, int wgt_shared, float* out_mean, float* out_median,
                                       float* out_cov, float cov_min, float valid_min, const float* trans_tf,
                                       const float* rot_tf, int batch, int n, int H, int W, int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(y && wgt && trans_tf && rot_tf, "asr_realign_covered_f32: null pointer");
    ASR_REQUIRE(out_mean || out_median || out_cov, "asr_realign_covered_f32: nothing to compute (out_mean, out_median and out_cov are NULL)");
    ASR_REQUIRE(batch > 0 && batch <= 65535 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "asr_realign_covered_f32: bad shape");
    ASR_REQUIRE(cov_min > 0.0f && cov_min < __builtin_inff(), "asr_realign_covered_f32: cov_min=%g must be finite and > 0", (double)cov_min);
    ASR_REQUIRE(valid_min > 0.0f && valid_min < __builtin_inff(), "asr_realign_covered_f32: valid_min=%g must be finite and > 0",
                (double)valid_min);
    ASR_UNSUPPORTED(out_median && n > kSelMaxCopies,
                    "asr_realign_covered_f32: n=%d copies with out_median, at most %d (256 bytes of LDS per copy, 160 KiB per workgroup)",
                    n, kSelMaxCopies);
    SrDims d;
    d.batch = batch; d.n = n; d.H = H; d.W = W; d.h = h; d.w = w; d.f = 0;
    SrCover cv;
    cv.cov_min = cov_min; cv.valid_min = valid_min; cv.wgt_stride = wgt_shared ? 0 : (int64_t)h * w;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipStream_t s = asr_stream(stream);
    if (!out_median) {
        hipLaunchKernelGGL(sr_realign_covered_kernel, hr_grid(d), kBlock, 0, s, y, wgt, out_mean, out_cov, trans_tf, rot_tf, d, cv, sy, sx);
        ASR_LAUNCH_CHECK();
        return ASR_OK;
    }
    const int64_t tiles_x = asr_cdiv(W, kSelX), tiles = tiles_x * asr_cdiv(H, kSelY);
    ASR_REQUIRE(tiles <= 0x7fffffff, "asr_realign_covered_f32: %dx%d output exceeds the grid", H, W);
    const size_t lds = sizeof(unsigned) * (size_t)n * kSelPix;
    static AsrDeviceOnce once;
    if (lds > 64 * 1024)
        ASR_HIP_CHECK(asr_allow_dynamic_lds(once, reinterpret_cast<const void*>(sr_realign_covered_median_kernel), kSelLdsMax));
    hipLaunchKernelGGL(sr_realign_covered_median_kernel, dim3((unsigned)tiles, 1, (unsigned)batch), dim3(kSelX, kSelY), lds, s,
                       y, wgt, out_mean, out_median, out_cov, trans_tf, rot_tf, d, cv, (int)tiles_x, sy, sx);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_realign_moments_f32(const float* y, const float* wgt, int wgt_shared, float* out_mean, float* out_var,
                                       float* out_nv, float valid_min, const float* trans_tf, const float* rot_tf, int batch,
                                       int n, int H, int W, int h, int w, asr_stream_t stream) {
    ASR_REQUIRE(y && trans_tf && rot_tf, "asr_realign_moments_f32: null pointer");
    ASR_REQUIRE(out_mean || out_var || out_nv, "asr_realign_moments_f32: nothing to compute (out_mean, out_var and out_nv are NULL)");
    ASR_REQUIRE(batch > 0 && batch <= 65535 && n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "asr_realign_moments_f32: bad shape");
    ASR_REQUIRE(!wgt || (valid_min > 0.0f && valid_min < __builtin_inff()),
                "asr_realign_moments_f32: valid_min=%g must be finite and > 0", (double)valid_min);
    SrDims d;
    d.batch = batch; d.n = n; d.H = H; d.W = W; d.h = h; d.w = w; d.f = 0;
    SrCover cv;
    cv.cov_min = 0.0f; cv.valid_min = valid_min; cv.wgt_stride = wgt_shared ? 0 : (int64_t)h * w;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipStream_t s = asr_stream(stream);
    if (wgt)
        hipLaunchKernelGGL(sr_realign_moments_kernel<true>, hr_grid(d), kBlock, 0, s, y, wgt, out_mean, out_var, out_nv, trans_tf,
                           rot_tf, d, cv, sy, sx);
    else
        hipLaunchKernelGGL(sr_realign_moments_kernel<false>, hr_grid(d), kBlock, 0, s, y, wgt, out_mean, out_var, out_nv, trans_tf,
                           rot_tf, d, cv, sy, sx);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

#ifdef ASR_DIAG_KFWD_CHECK
// diag builds only: copy out (and clear) K_fwd's self-check counters [128] and records [16][12]
extern "C" int asr_diag_kfwd_read(unsigned* counters, float* records) {
    ASR_HIP_CHECK(hipDeviceSynchronize());
    ASR_HIP_CHECK(hipMemcpyFromSymbol(counters, HIP_SYMBOL(g_kfwd_cnt), sizeof(unsigned) * 128));
    ASR_HIP_CHECK(hipMemcpyFromSymbol(records, HIP_SYMBOL(g_kfwd_rec), sizeof(float) * 16 * 12));
    static unsigned zero[128];
    ASR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_kfwd_cnt), zero, sizeof(zero)));
    return ASR_OK;
}
#endif
