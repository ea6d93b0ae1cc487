// Windowed dense CRF over classes and image (mean field, Potts compatibility, exact message passing inside a dilated window, as
// in ConvCRF) -- the rule is in include/asr_hip.h, section "windowed CRF".
//
// Kernels:
//   crf_unaries_scores_kernel  K score planes and their maxima -> L = K + 1 unary planes
//   crf_unaries_labels_kernel  an int32 label map -> L unary planes
//   crf_init_kernel            Q^0 = softmax(z); with T = 0 also the labels (argmax of z)
//   crf_step_kernel<LC>        one iteration: Q^{t-1} -> the logits s, Q^t = softmax(s); the last one writes the labels
// One launch per iteration on the caller's stream; no workgroup ever waits for another, no atomics.
// crf_step_kernel: a workgroup of 1024 threads owns a 32 x 32 tile, one pixel per thread (a wave is two tile rows of 32 lanes,
// so a 4-byte LDS read of a wave's half touches 32 consecutive floats: conflict-free at any row stride).  It stages the guide
// tile with its r d halo in LDS once, then the Q planes with halo in chunks of LC labels, zeros outside the image.  The offset
// loop is outermost within a chunk: the appearance weight a (one expf) and the smoothness weight g (a table in LDS, built once
// per workgroup) are computed once per (pixel, offset, chunk) and the chunk's 2 LC sums stay in registers.  A neighbour outside
// the image gets weight 0 in the sums AND in the normalisers (the window is clipped); offsets are added in ascending (dy, dx).
// The logits of all L labels do not fit registers at a run-time L without indexing them dynamically (scratch), so a thread
// parks its own logits in the destination Q plane, keeps the running maximum and its label, and then turns its own L values
// into the softmax in place: nobody else reads the destination buffer during the launch (ping-pong).
#include "asr_common.h"

#include <math.h>

namespace {

constexpr int CRF_T = 32;                                   // tile edge (output pixels)
constexpr int CRF_THREADS = CRF_T * CRF_T;                  // one pixel per thread: (x, y) = (tid & 31, tid >> 5)
constexpr int CRF_RMAX = 7;                                 // radius cap
constexpr int CRF_HALO_MAX = 16;                            // cap of radius * dilation
constexpr int CRF_TMAX = 32;                                // iteration cap
constexpr int CRF_LMAX = ASR_MAX_CLASS_SET;                 // label cap (label 0 + at most 31 ids)
constexpr int CRF_TAPS = (2 * CRF_RMAX + 1) * (2 * CRF_RMAX + 1);
constexpr int CRF_STAGE = 2;                                // staging loads in flight per thread
constexpr float CRF_EXP_MIN = -80.0f;                       // exponent clamp: every weight stays a normal f32 number
constexpr int CRF_TAB = (2 * CRF_TAPS + 3) & ~3;            // floats of the two per-offset tables at the head of the LDS (16-byte multiple)
constexpr size_t CRF_LDS_BUDGET = 160 * 1024;               // a CU's LDS

struct CrfParams {
    int r, d;
    float w_app, w_smooth;
    float inv_pos, inv_rgb, inv_smooth;                     // 1 / (2 theta^2), from the host in double, rounded once
};

__host__ __device__ inline int crf_region(int halo) { return CRF_T + 2 * halo; }
// a staged plane has RW rows of RW + 1 floats (odd: lanes that walk down a column while staging meet distinct banks)
inline size_t crf_plane_floats(int halo) { return (size_t)crf_region(halo) * (crf_region(halo) + 1); }
inline size_t crf_lds_bytes(int chunk, int halo) { return sizeof(float) * (CRF_TAB + (3 + chunk) * crf_plane_floats(halo)); }

// Position idx of the RW x RW region whose corner is image pixel (x0, y0) -> the image pixel to load (the nearest one inside:
// the load is unconditional), whether the position lies in the image, and where it lives in a staged plane.
__device__ __forceinline__ size_t crf_stage_pixel(int idx, int RW, int x0, int y0, int H, int W, bool& inside, int& lds) {
    const int ry = idx / RW, rx = idx - ry * RW, gy = y0 + ry, gx = x0 + rx;
    lds = ry * (RW + 1) + rx;
    inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
    return (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
}

// buf[l * HW], l = 0 .. L-1: this thread's logits, written by itself -> softmax with the maximum m subtracted, in place
__device__ __forceinline__ void crf_softmax_inplace(float* buf, size_t HW, int L, float m) {
    float sum = 0.0f;
    for (int l = 0; l < L; ++l) sum += expf(buf[l * HW] - m);
    for (int l = 0; l < L; ++l) buf[l * HW] = expf(buf[l * HW] - m) / sum;
}

__global__ __launch_bounds__(256) void crf_unaries_scores_kernel(const float* __restrict__ scores,
                                                                 const float* __restrict__ seg_minmax, float* __restrict__ z,
                                                                 int64_t pixels, float th_factor, float tau) {
    const int l = blockIdx.y;                               // plane of z; l >= 1: class l - 1
    const float th = l ? seg_minmax[(l - 1) * 2 + 1] * th_factor : 0.0f;      // asr_fuse_labels_f32's f32 product
    const float* s = scores + (int64_t)(l ? l - 1 : 0) * pixels;
    float* out = z + (int64_t)l * pixels;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256)
        out[i] = l ? (s[i] - th) / tau : 0.0f;
}

__global__ __launch_bounds__(256) void crf_unaries_labels_kernel(const int32_t* __restrict__ labels, float* __restrict__ z,
                                                                 int64_t pixels, int L, float log_hit, float log_miss,
                                                                 AsrClassSet set) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
        const int v = labels[i];
        int hit = v == 0 ? 0 : -1;                          // the label l whose id the map holds, -1: none of them
        for (int k = 0; k < L - 1; ++k)
            if (v == set.id[k]) hit = k + 1;
        for (int l = 0; l < L; ++l) z[(int64_t)l * pixels + i] = hit < 0 ? 0.0f : (l == hit ? log_hit : log_miss);
    }
}

__global__ __launch_bounds__(256) void crf_init_kernel(const float* __restrict__ z, float* __restrict__ q,
                                                       int32_t* __restrict__ labels, size_t HW, int L, AsrClassSet set) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    float m = z[p];
    int lab = 0;
    for (int l = 1; l < L; ++l) {
        const float v = z[l * HW + p];
        if (v > m) { m = v; lab = set.id[l - 1]; }          // strict: equal values stay with the lowest l
    }
    if (labels) labels[p] = lab;
    if (q) {
        float sum = 0.0f;
        for (int l = 0; l < L; ++l) sum += expf(z[l * HW + p] - m);
        for (int l = 0; l < L; ++l) q[l * HW + p] = expf(z[l * HW + p] - m) / sum;
    }
}

// (no occupancy pin: held at 64 registers the 8-label instantiation spills to scratch; left alone it takes 76, which is one
// 16-wave workgroup per CU, and the 4-label one 59, which is two)
template <int LC>
__global__ __launch_bounds__(CRF_THREADS) void crf_step_kernel(
    const float* __restrict__ guide, const float* __restrict__ z, const float* __restrict__ src, float* dst,
    int32_t* __restrict__ labels, int H, int W, int L, CrfParams prm, AsrClassSet set) {
    extern __shared__ __align__(16) float crf_lds[];
    float* tab_pos = crf_lds;                               // per offset: -delta^2 / (2 theta_pos^2) ...
    float* tab_g = crf_lds + CRF_TAPS;                      // ... and g
    const int r = prm.r, d = prm.d, halo = r * d, n = 2 * r + 1;
    const int RW = crf_region(halo), RS = RW + 1, CS = RW * RS, RR = RW * RW;
    float* gI = crf_lds + CRF_TAB;                          // [3][RW][RS]: the guide
    float* qs = gI + 3 * CS;                                // [LC][RW][RS]: Q^{t-1} of the chunk's labels
    const int tid = threadIdx.x, tx = tid & (CRF_T - 1), ty = tid / CRF_T;
    const int tx0 = blockIdx.x * CRF_T, ty0 = blockIdx.y * CRF_T;
    const size_t HW = (size_t)H * W;
    if (tid < n * n) {
        const int dy = tid / n - r, dx = tid % n - r;
        const float d2 = (float)(d * d * (dy * dy + dx * dx));
        tab_pos[tid] = -(d2 * prm.inv_pos);
        tab_g[tid] = expf(fmaxf(-(d2 * prm.inv_smooth), CRF_EXP_MIN));
    }
    for (int base = 0; base < RR; base += CRF_STAGE * CRF_THREADS) {
        float v[CRF_STAGE][3];
        bool ok[CRF_STAGE];
        int at[CRF_STAGE];
#pragma unroll
        for (int u = 0; u < CRF_STAGE; ++u) {
            const float* g = guide + 3 * crf_stage_pixel(base + u * CRF_THREADS + tid, RW, tx0 - halo, ty0 - halo, H, W, ok[u], at[u]);
            v[u][0] = g[0]; v[u][1] = g[1]; v[u][2] = g[2];
        }
#pragma unroll
        for (int u = 0; u < CRF_STAGE; ++u) {
            if (base + u * CRF_THREADS + tid < RR) {        // (a position outside the image is never read with weight: any value)
                gI[at[u]] = ok[u] ? v[u][0] : 0.0f;
                gI[CS + at[u]] = ok[u] ? v[u][1] : 0.0f;
                gI[2 * CS + at[u]] = ok[u] ? v[u][2] : 0.0f;
            }
        }
    }
    const int y = ty0 + ty, x = tx0 + tx;
    const bool live = y < H && x < W;                       // the others compute on in-bounds LDS and write nothing
    const size_t p = (size_t)min(y, H - 1) * W + min(x, W - 1);
    const int ctr = (ty + halo) * RS + tx + halo;
    float m = 0.0f;                                         // running maximum of the logits, and its label's id
    int lab = 0;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int l0 = 0; l0 < L; l0 += LC) {
        if (l0) __syncthreads();                            // the previous chunk's reads are done
        for (int idx = tid; idx < RR; idx += CRF_THREADS) {    // one position per trip: its LC loads are in flight together
            bool ok;
            int at;
            const float* s = src + crf_stage_pixel(idx, RW, tx0 - halo, ty0 - halo, H, W, ok, at);
            float v[LC];
#pragma unroll
            for (int j = 0; j < LC; ++j) v[j] = s[(size_t)min(l0 + j, L - 1) * HW];
#pragma unroll
            for (int j = 0; j < LC; ++j) qs[j * CS + at] = (ok && l0 + j < L) ? v[j] : 0.0f;
        }
        __syncthreads();                                    // guide, tables and the chunk's planes are in LDS
        if (l0 == 0) { c0 = gI[ctr]; c1 = gI[CS + ctr]; c2 = gI[2 * CS + ctr]; }
        float A[LC], G[LC], na = 0.0f, ng = 0.0f;
#pragma unroll
        for (int j = 0; j < LC; ++j) A[j] = G[j] = 0.0f;
        int o = 0;
        for (int dy = -r; dy <= r; ++dy) {
            const int qy = y + d * dy;
            const bool yin = qy >= 0 && qy < H;
            for (int dx = -r; dx <= r; ++dx, ++o) {
                if (dy == 0 && dx == 0) continue;
                const int off = ctr + d * (dy * RS + dx);   // inside the region for every thread: |d dy|, |d dx| <= halo
                const int qx = x + d * dx;
                const bool in = yin && qx >= 0 && qx < W;
                const float e0 = gI[off] - c0, e1 = gI[CS + off] - c1, e2 = gI[2 * CS + off] - c2;
                const float dist2 = e0 * e0 + e1 * e1 + e2 * e2;
                const float a = in ? expf(fmaxf(tab_pos[o] - dist2 * prm.inv_rgb, CRF_EXP_MIN)) : 0.0f;
                const float g = in ? tab_g[o] : 0.0f;
                na += a;
                ng += g;
#pragma unroll
                for (int j = 0; j < LC; ++j) {
                    const float qv = qs[j * CS + off];
                    A[j] += a * qv;
                    G[j] += g * qv;
                }
            }
        }
        float zr[LC];                                       // loaded here, not held across the offset loop
#pragma unroll
        for (int j = 0; j < LC; ++j) zr[j] = z[(size_t)min(l0 + j, L - 1) * HW + p];
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            const int l = l0 + j;
            if (live && l < L) {
                // a pixel without neighbours (the 1 x 1 image) has both terms equal to 0
                const float s = zr[j] + prm.w_app * (na > 0.0f ? A[j] / na : 0.0f) + prm.w_smooth * (ng > 0.0f ? G[j] / ng : 0.0f);
                if (dst) dst[l * HW + p] = s;
                if (l == 0) { m = s; lab = 0; }
                else if (s > m) { m = s; lab = set.id[l - 1]; }                 // strict: equal values stay with the lowest l
            }
        }
    }
    if (live) {
        if (labels) labels[p] = lab;
        if (dst) crf_softmax_inplace(dst + p, HW, L, m);
    }
}

AsrDeviceOnce g_step4_lds, g_step8_lds;

int crf_check_shape(const char* fn, int L, int H, int W) {
    ASR_REQUIRE(H >= 1 && W >= 1, "%s: bad shape H=%d W=%d", fn, H, W);
    ASR_REQUIRE(L >= 2, "%s: %d labels (label 0 and at least one class: 2..%d)", fn, L, CRF_LMAX);
    ASR_UNSUPPORTED(L > CRF_LMAX, "%s: %d labels above the cap of %d", fn, L, CRF_LMAX);
    return ASR_OK;
}

int crf_check_config(const char* fn, const asr_crf_config* c) {
    ASR_REQUIRE(c->radius >= 1, "%s: radius %d below 1", fn, c->radius);
    ASR_REQUIRE(c->dilation >= 1, "%s: dilation %d below 1", fn, c->dilation);
    ASR_REQUIRE(c->iterations >= 0, "%s: %d iterations", fn, c->iterations);
    ASR_REQUIRE(isfinite(c->w_app) && c->w_app >= 0.0f, "%s: w_app must be finite and >= 0 (got %g)", fn, (double)c->w_app);
    ASR_REQUIRE(isfinite(c->w_smooth) && c->w_smooth >= 0.0f, "%s: w_smooth must be finite and >= 0 (got %g)", fn,
                (double)c->w_smooth);
    ASR_REQUIRE(isfinite(c->theta_pos) && c->theta_pos > 0.0f, "%s: theta_pos must be finite and > 0 (got %g)", fn,
                (double)c->theta_pos);
    ASR_REQUIRE(isfinite(c->theta_rgb) && c->theta_rgb > 0.0f, "%s: theta_rgb must be finite and > 0 (got %g)", fn,
                (double)c->theta_rgb);
    ASR_REQUIRE(isfinite(c->theta_smooth) && c->theta_smooth > 0.0f, "%s: theta_smooth must be finite and > 0 (got %g)", fn,
                (double)c->theta_smooth);
    ASR_UNSUPPORTED(c->radius > CRF_RMAX, "%s: radius %d above the cap of %d", fn, c->radius, CRF_RMAX);
    ASR_UNSUPPORTED((int64_t)c->radius * c->dilation > CRF_HALO_MAX,
                    "%s: radius %d x dilation %d above the cap of %d (a 32 x 32 tile and its halo must fit a CU's LDS)", fn,
                    c->radius, c->dilation, CRF_HALO_MAX);
    ASR_UNSUPPORTED(c->iterations > CRF_TMAX, "%s: %d iterations above the cap of %d", fn, c->iterations, CRF_TMAX);
    return ASR_OK;
}

float crf_inv_two_sq(float theta) { return (float)(1.0 / (2.0 * (double)theta * (double)theta)); }

unsigned crf_flat_grid(int64_t pixels) { return (unsigned)(asr_cdiv(pixels, 256) < 65535 ? asr_cdiv(pixels, 256) : 65535); }

}  // namespace

extern "C" size_t asr_crf_workspace_bytes(int L, int H, int W) {
    if (L < 2 || L > CRF_LMAX || H < 1 || W < 1) return 0;
    return sizeof(float) * 2 * (size_t)L * (size_t)H * (size_t)W;
}

extern "C" int asr_crf_unaries_scores_f32(const float* scores, float* minmax_ws, float* z, int64_t pixels, int K, float th_factor,
                                          float tau, asr_stream_t stream) {
    ASR_REQUIRE(scores && minmax_ws && z, "asr_crf_unaries_scores_f32: null pointer");
    ASR_REQUIRE(pixels > 0, "asr_crf_unaries_scores_f32: bad shape");
    ASR_REQUIRE(K >= 1, "asr_crf_unaries_scores_f32: %d score planes (1..%d)", K, CRF_LMAX - 1);
    ASR_UNSUPPORTED(K > CRF_LMAX - 1, "asr_crf_unaries_scores_f32: %d score planes above the cap of %d", K, CRF_LMAX - 1);
    ASR_REQUIRE(isfinite(th_factor), "asr_crf_unaries_scores_f32: th_factor must be finite (got %g)", (double)th_factor);
    ASR_REQUIRE(isfinite(tau) && tau > 0.0f, "asr_crf_unaries_scores_f32: tau must be finite and > 0 (got %g)", (double)tau);
    const int rc = asr_minmax_f32(scores, minmax_ws, pixels, K, stream);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(crf_unaries_scores_kernel, dim3(crf_flat_grid(pixels), (unsigned)(K + 1)), dim3(256), 0, asr_stream(stream),
                       scores, (const float*)minmax_ws, z, pixels, th_factor, tau);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_crf_unaries_labels_f32(const int32_t* labels, float* z, int64_t pixels, const int* ids, int L, float conf,
                                          asr_stream_t stream) {
    ASR_REQUIRE(labels && z, "asr_crf_unaries_labels_f32: null pointer");
    ASR_REQUIRE(pixels > 0, "asr_crf_unaries_labels_f32: bad shape");
    int rc = crf_check_shape("asr_crf_unaries_labels_f32", L, 1, 1);
    if (rc != ASR_OK) return rc;
    AsrClassSet set;
    rc = asr_label_set("asr_crf_unaries_labels_f32", ids, L - 1, 0, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(conf > 1.0f / (float)L && conf < 1.0f, "asr_crf_unaries_labels_f32: conf must lie in (1/%d, 1) (got %g)", L,
                (double)conf);
    const float log_hit = (float)log((double)conf), log_miss = (float)log((1.0 - (double)conf) / (double)(L - 1));
    hipLaunchKernelGGL(crf_unaries_labels_kernel, dim3(crf_flat_grid(pixels)), dim3(256), 0, asr_stream(stream), labels, z, pixels,
                       L, log_hit, log_miss, set);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_crf_refine_f32(const float* guide, const float* z, const int* ids, int L, int H, int W,
                                  const asr_crf_config* cfg, void* workspace, int32_t* labels, float* q_out,
                                  asr_stream_t stream) {
    ASR_REQUIRE(guide && z && cfg && workspace && labels, "asr_crf_refine_f32: null pointer");
    int rc = crf_check_shape("asr_crf_refine_f32", L, H, W);
    if (rc != ASR_OK) return rc;
    AsrClassSet set;
    rc = asr_label_set("asr_crf_refine_f32", ids, L - 1, 0, &set);
    if (rc != ASR_OK) return rc;
    rc = crf_check_config("asr_crf_refine_f32", cfg);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(((uintptr_t)workspace & 3) == 0, "asr_crf_refine_f32: workspace not aligned to 4 bytes");
    if (q_out) {                                            // the launches read z while they park logits in q_out
        const uintptr_t zb = (uintptr_t)z, qb = (uintptr_t)q_out, span = sizeof(float) * (uintptr_t)L * (uintptr_t)H * (uintptr_t)W;
        ASR_REQUIRE(qb + span <= zb || zb + span <= qb, "asr_crf_refine_f32: q_out must not overlap z");
    }
    const int T = cfg->iterations, halo = cfg->radius * cfg->dilation;
    const size_t HW = (size_t)H * W;
    hipStream_t s = asr_stream(stream);
    float* buf[2] = {(float*)workspace, (float*)workspace + (size_t)L * HW};
    const unsigned init_grid = (unsigned)asr_cdiv((int64_t)HW, 256);
    ASR_REQUIRE(asr_cdiv((int64_t)HW, 256) <= 0x7fffffff, "asr_crf_refine_f32: image of %d x %d too large", H, W);
    if (T == 0) {
        hipLaunchKernelGGL(crf_init_kernel, dim3(init_grid), dim3(256), 0, s, z, q_out, labels, HW, L, set);
        ASR_LAUNCH_CHECK();
        return ASR_OK;
    }
    // eight labels per chunk where the planes fit the LDS and there are that many, else four
    const bool wide = L > 4 && crf_lds_bytes(8, halo) <= CRF_LDS_BUDGET;
    const size_t lds = crf_lds_bytes(wide ? 8 : 4, halo);
    if (wide)
        ASR_HIP_CHECK(asr_allow_dynamic_lds(g_step8_lds, (const void*)crf_step_kernel<8>, (int)CRF_LDS_BUDGET));
    else
        ASR_HIP_CHECK(asr_allow_dynamic_lds(g_step4_lds, (const void*)crf_step_kernel<4>, (int)CRF_LDS_BUDGET));
    CrfParams prm;
    prm.r = cfg->radius; prm.d = cfg->dilation;
    prm.w_app = cfg->w_app; prm.w_smooth = cfg->w_smooth;
    prm.inv_pos = crf_inv_two_sq(cfg->theta_pos); prm.inv_rgb = crf_inv_two_sq(cfg->theta_rgb);
    prm.inv_smooth = crf_inv_two_sq(cfg->theta_smooth);
    hipLaunchKernelGGL(crf_init_kernel, dim3(init_grid), dim3(256), 0, s, z, buf[0], (int32_t*)nullptr, HW, L, set);
    ASR_LAUNCH_CHECK();
    const dim3 grid((unsigned)asr_cdiv(W, CRF_T), (unsigned)asr_cdiv(H, CRF_T));
    for (int t = 1; t <= T; ++t) {
        const float* src = buf[(t - 1) & 1];
        float* dst = t == T ? q_out : buf[t & 1];           // the last iteration: Q only if asked, and the labels
        int32_t* lab = t == T ? labels : nullptr;
        if (wide)
            hipLaunchKernelGGL(crf_step_kernel<8>, grid, dim3(CRF_THREADS), lds, s, guide, z, src, dst, lab, H, W, L, prm, set);
        else
            hipLaunchKernelGGL(crf_step_kernel<4>, grid, dim3(CRF_THREADS), lds, s, guide, z, src, dst, lab, H, W, L, prm, set);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}
