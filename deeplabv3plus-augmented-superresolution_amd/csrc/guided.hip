// Guided filter with a colour guide (He, Sun, Tang) for [P, H, W] score planes -- the rule is in include/asr_hip.h.
//
// Three kernels share one tile scheme and one window-sum routine:
//   guided_prepare_kernel  guide -> per pixel the window mean of the guide and the LDL^T factor of (S + eps U)   (once per image)
//   guided_ab_kernel       p, guide, state -> a (3) and b per pixel and plane, into the workspace
//   guided_q_kernel        window means of a and b, q = mean(a) . I + mean(b)
// A workgroup of 256 threads owns a GF_T x GF_T tile of output pixels and stages the tile plus an r-wide halo in LDS, zeros
// outside the image (the windows are CLIPPED: a zero adds nothing, and the pixel count N_k is arithmetic).  The (2r+1)^2 sums
// are separable inside the tile: first along the rows into a [RW][GF_T] buffer, then down the columns.  Every sum adds its
// 2r+1 terms directly, in ascending order -- no running sums, no summed-area table -- so a term's rounding error never
// outlives its window; what neighbouring sums share is the READ: a thread forms four adjacent sums from the 2r+4 values they
// cover (gf_slide4).  The kernels are bound by vector instructions, not by LDS or HBM bandwidth, and that sharing is what cuts
// them.  The channels of one pass go through the row-sum buffer one after the other, which is what lets a 32 x 32 tile keep
// its 96 x 96 region at r = 32 within a CU's LDS: 4 * (4 * 96 * 97 + 96 * 33) = 161 664 bytes.
// The guide is centred per tile on the guide value at the tile's centre pixel before any product is formed: covariances do
// not change with a shift, and the shifted values are small where the guide is smooth, which is where S cancels worst.
// No atomics; a plane is a grid layer (blockIdx.z) that runs the same statements whatever P is.
#include "asr_common.h"

#include <math.h>

namespace {

constexpr int GF_T = 32;                                   // tile edge (output pixels)
constexpr int GF_THREADS = 256;
constexpr int GF_OWN = GF_T * GF_T / GF_THREADS;           // output pixels per thread: (x, 4 g + k), k = 0..3, x = tid & 31, g = tid >> 5
constexpr int GF_HS = GF_T + 1;                            // row stride of the row-sum buffer: odd, so lanes that walk down a column meet 32 banks
constexpr int GF_RMAX = 32;
constexpr int GF_STATE = 9;                                // planes of the state: centred guide mean (3), l10 l20 l21, 1/d0 1/d1 1/d2
static_assert(GF_OWN == 4, "gf_slide4 forms four sums per thread");

// Region edge RW = GF_T + 2r (even); a staged channel has rows of RW + 1 floats (odd, as GF_HS) and RW rows.
__host__ __device__ inline int gf_region(int r) { return GF_T + 2 * r; }
inline size_t gf_lds_bytes(int channels, int r) {
    const size_t rw = gf_region(r);
    return sizeof(float) * (channels * rw * (rw + 1) + rw * GF_HS);
}

// pixels of the clipped window round i on an axis of n
__device__ __forceinline__ int gf_count(int i, int n, int r) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// Staging a region: position idx of the RW x RW region whose corner is image pixel (x0, y0) -> the image pixel to load, and
// whether the position lies in the image.  A position outside (or past the region's end) loads the nearest pixel inside
// instead and is stored as zero, at offset lds of each channel: the loads are unconditional, so GF_STAGE of them are in flight per thread before the first
// value is needed.
constexpr int GF_STAGE = 4;
__device__ __forceinline__ size_t gf_stage_pixel(int idx, int RW, int x0, int y0, int H, int W, bool& inside, int& lds) {
    const int ry = idx / RW, rx = idx - ry * RW, gy = y0 + ry, gx = x0 + rx;
    lds = ry * (RW + 1) + rx;                               // where the position lives in a staged channel
    inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
    return (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
}

// The guide value every pixel of this tile is centred on.
__device__ __forceinline__ void gf_centre(const float* __restrict__ guide, int H, int W, int tx0, int ty0, float c[3]) {
    const int cy = min(ty0 + GF_T / 2, H - 1), cx = min(tx0 + GF_T / 2, W - 1);
    const float* g = guide + ((size_t)cy * W + cx) * 3;
    c[0] = g[0]; c[1] = g[1]; c[2] = g[2];
}

// Four adjacent window sums from the n + 3 values get(0) .. get(n + 2) they cover: sum k adds get(k) .. get(k + n - 1), in that
// order.  Each value is read once.
template <class G>
__device__ __forceinline__ void gf_slide4(G get, int n, float a[4]) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (n >= 3) {                                           // r >= 1: head, body (all four sums, no predicates), tail
        float v = get(0);              a0 += v;
        v = get(1);                    a0 += v; a1 += v;
        v = get(2);                    a0 += v; a1 += v; a2 += v;
#pragma unroll 4
        for (int j = 3; j < n; ++j) {                       // unrolled: the LDS reads of four steps are in flight together
            v = get(j);                a0 += v; a1 += v; a2 += v; a3 += v;
        }
        v = get(n);                    a1 += v; a2 += v; a3 += v;
        v = get(n + 1);                a2 += v; a3 += v;
        v = get(n + 2);                a3 += v;
    } else {                                                // r = 0: each sum is its one value
        a0 += get(0); a1 += get(1); a2 += get(2); a3 += get(3);
    }
    a[0] = a0; a[1] = a1; a[2] = a2; a[3] = a3;
}

// Window sums of one channel for the thread's GF_OWN pixels.  f(off) is the channel's value at offset off = row * (RW + 1) + col
// of the staged region (region row = tile row + r).  Row sums first: a thread takes four adjacent tile columns of one region
// row, and its lanes walk down the rows (odd row strides: conflict-free); then column sums out of hs, four adjacent tile rows
// per thread, lanes along the row.  Ends with a barrier: hs is free again.  The caller has a barrier between staging the region
// and the first call.
template <class F>
__device__ __forceinline__ void gf_window_sums(F f, float* __restrict__ hs, int r, int RW, float out[GF_OWN]) {
    const int tid = threadIdx.x, n = 2 * r + 1;
    const int RWp = (RW + 31) & ~31;
    for (int idx = tid; idx < (GF_T / 4) * RWp; idx += GF_THREADS) {
        const int row = idx % RWp, x0 = (idx / RWp) * 4;
        if (row < RW) {
            const int base = row * (RW + 1) + x0;
            float a[4];
            gf_slide4([=](int j) { return f(base + j); }, n, a);
            float* dst = hs + row * GF_HS + x0;
            dst[0] = a[0]; dst[1] = a[1]; dst[2] = a[2]; dst[3] = a[3];
        }
    }
    __syncthreads();
    const float* col = hs + 4 * (tid >> 5) * GF_HS + (tid & 31);
    gf_slide4([=](int j) { return col[j * GF_HS]; }, n, out);
    __syncthreads();
}

__global__ __launch_bounds__(GF_THREADS) void guided_prepare_kernel(const float* __restrict__ guide, float* __restrict__ state,
                                                                    int H, int W, int r, float eps) {
    extern __shared__ __align__(16) float gf_lds[];
    const int RW = gf_region(r), RR = RW * RW, CS = RW * (RW + 1);       // region positions, floats per staged channel
    float* in = gf_lds;                                     // [3][RW][RW + 1]: the centred guide
    float* hs = gf_lds + 3 * CS;                            // [RW][GF_HS]
    const int tid = threadIdx.x, tx0 = blockIdx.x * GF_T, ty0 = blockIdx.y * GF_T;
    float c[3];
    gf_centre(guide, H, W, tx0, ty0, c);
    for (int base = 0; base < RR; base += GF_STAGE * GF_THREADS) {
        float v[GF_STAGE][3];
        bool ok[GF_STAGE];
        int at[GF_STAGE];
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            const size_t pix = gf_stage_pixel(base + u * GF_THREADS + tid, RW, tx0 - r, ty0 - r, H, W, ok[u], at[u]);
            const float* g = guide + pix * 3;
            v[u][0] = g[0]; v[u][1] = g[1]; v[u][2] = g[2];
        }
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            if (base + u * GF_THREADS + tid < RR) {
                in[at[u]] = ok[u] ? v[u][0] - c[0] : 0.0f;
                in[CS + at[u]] = ok[u] ? v[u][1] - c[1] : 0.0f;
                in[2 * CS + at[u]] = ok[u] ? v[u][2] - c[2] : 0.0f;
            }
        }
    }
    __syncthreads();
    float s1[3][GF_OWN], s2[6][GF_OWN];                     // sums of J_c, and of J0J0 J0J1 J0J2 J1J1 J1J2 J2J2
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float* pa = in + a * CS;
        gf_window_sums([=](int off) { return pa[off]; }, hs, r, RW, s1[a]);
    }
    {
        int m = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b, ++m) {
                const float* pa = in + a * CS;
                const float* pb = in + b * CS;
                gf_window_sums([=](int off) { return pa[off] * pb[off]; }, hs, r, RW, s2[m]);
            }
    }
    const size_t HW = (size_t)H * W;
#pragma unroll
    for (int k = 0; k < GF_OWN; ++k) {
        const int y = ty0 + 4 * (tid >> 5) + k, x = tx0 + (tid & 31);
        if (y >= H || x >= W) continue;
        const float N = (float)(gf_count(y, H, r) * gf_count(x, W, r));
        const float m0 = s1[0][k] / N, m1 = s1[1][k] / N, m2 = s1[2][k] / N;
        const float A = s2[0][k] / N - m0 * m0 + eps, B = s2[1][k] / N - m0 * m1, C = s2[2][k] / N - m0 * m2;
        const float D = s2[3][k] / N - m1 * m1 + eps, E = s2[4][k] / N - m1 * m2, F = s2[5][k] / N - m2 * m2 + eps;
        // (S + eps U) = L diag(d) L^T, no pivoting (symmetric positive definite); a = (S + eps U)^-1 c is then two triangular
        // solves in guided_ab_kernel, backward stable where an explicit inverse's determinant would cancel twice
        const float d0 = A, l10 = B / d0, l20 = C / d0;
        const float d1 = D - l10 * B, t = E - l20 * B, l21 = t / d1;
        const float d2 = F - l20 * C - l21 * t;
        float* st = state + (size_t)y * W + x;
        st[0] = m0; st[HW] = m1; st[2 * HW] = m2;
        st[3 * HW] = l10; st[4 * HW] = l20; st[5 * HW] = l21;
        st[6 * HW] = 1.0f / d0; st[7 * HW] = 1.0f / d1; st[8 * HW] = 1.0f / d2;
    }
}

__global__ __launch_bounds__(GF_THREADS) void guided_ab_kernel(const float* __restrict__ state, const float* __restrict__ guide,
                                                               const float* __restrict__ p, float* __restrict__ ab, int H, int W,
                                                               int r) {
    extern __shared__ __align__(16) float gf_lds[];
    const int RW = gf_region(r), RR = RW * RW, CS = RW * (RW + 1);       // region positions, floats per staged channel
    float* in = gf_lds;                                     // [4][RW][RW + 1]: p, p J0, p J1, p J2
    float* hs = gf_lds + 4 * CS;
    const int tid = threadIdx.x, tx0 = blockIdx.x * GF_T, ty0 = blockIdx.y * GF_T;
    const size_t HW = (size_t)H * W;
    p += blockIdx.z * HW;
    ab += blockIdx.z * 4 * HW;
    float c[3];
    gf_centre(guide, H, W, tx0, ty0, c);
    for (int base = 0; base < RR; base += GF_STAGE * GF_THREADS) {
        float v[GF_STAGE][4];
        bool ok[GF_STAGE];
        int at[GF_STAGE];
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            const size_t pix = gf_stage_pixel(base + u * GF_THREADS + tid, RW, tx0 - r, ty0 - r, H, W, ok[u], at[u]);
            const float* g = guide + pix * 3;
            v[u][0] = p[pix]; v[u][1] = g[0]; v[u][2] = g[1]; v[u][3] = g[2];
        }
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            if (base + u * GF_THREADS + tid < RR) {
                const float pv = ok[u] ? v[u][0] : 0.0f;
                in[at[u]] = pv;
                in[CS + at[u]] = ok[u] ? pv * (v[u][1] - c[0]) : 0.0f;
                in[2 * CS + at[u]] = ok[u] ? pv * (v[u][2] - c[1]) : 0.0f;
                in[3 * CS + at[u]] = ok[u] ? pv * (v[u][3] - c[2]) : 0.0f;
            }
        }
    }
    __syncthreads();
    float s[4][GF_OWN];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* pa = in + a * CS;
        gf_window_sums([=](int off) { return pa[off]; }, hs, r, RW, s[a]);
    }
#pragma unroll
    for (int k = 0; k < GF_OWN; ++k) {
        const int y = ty0 + 4 * (tid >> 5) + k, x = tx0 + (tid & 31);
        if (y >= H || x >= W) continue;
        const size_t pix = (size_t)y * W + x;
        const float* st = state + pix;
        const float N = (float)(gf_count(y, H, r) * gf_count(x, W, r));
        const float mu0 = st[0], mu1 = st[HW], mu2 = st[2 * HW];
        const float l10 = st[3 * HW], l20 = st[4 * HW], l21 = st[5 * HW];
        const float m = s[0][k] / N;
        const float z0 = s[1][k] / N - mu0 * m;
        const float z1 = (s[2][k] / N - mu1 * m) - l10 * z0;
        const float z2 = (s[3][k] / N - mu2 * m) - l20 * z0 - l21 * z1;
        const float a2 = z2 * st[8 * HW];
        const float a1 = z1 * st[7 * HW] - l21 * a2;
        const float a0 = z0 * st[6 * HW] - l10 * a1 - l20 * a2;
        // b = m - a . mu_I with mu_I = centred mean + centre
        const float b = m - a0 * (mu0 + c[0]) - a1 * (mu1 + c[1]) - a2 * (mu2 + c[2]);
        ab[pix] = a0; ab[HW + pix] = a1; ab[2 * HW + pix] = a2; ab[3 * HW + pix] = b;
    }
}

__global__ __launch_bounds__(GF_THREADS) void guided_q_kernel(const float* __restrict__ guide, const float* __restrict__ ab,
                                                              float* __restrict__ q, int H, int W, int r) {
    extern __shared__ __align__(16) float gf_lds[];
    const int RW = gf_region(r), RR = RW * RW, CS = RW * (RW + 1);       // region positions, floats per staged channel
    float* in = gf_lds;                                     // [4][RW][RW + 1]: a0, a1, a2, b
    float* hs = gf_lds + 4 * CS;
    const int tid = threadIdx.x, tx0 = blockIdx.x * GF_T, ty0 = blockIdx.y * GF_T;
    const size_t HW = (size_t)H * W;
    ab += blockIdx.z * 4 * HW;
    q += blockIdx.z * HW;
    for (int base = 0; base < RR; base += GF_STAGE * GF_THREADS) {
        float v[GF_STAGE][4];
        bool ok[GF_STAGE];
        int at[GF_STAGE];
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            const float* s = ab + gf_stage_pixel(base + u * GF_THREADS + tid, RW, tx0 - r, ty0 - r, H, W, ok[u], at[u]);
            v[u][0] = s[0]; v[u][1] = s[HW]; v[u][2] = s[2 * HW]; v[u][3] = s[3 * HW];
        }
#pragma unroll
        for (int u = 0; u < GF_STAGE; ++u) {
            if (base + u * GF_THREADS + tid < RR) {
                in[at[u]] = ok[u] ? v[u][0] : 0.0f;
                in[CS + at[u]] = ok[u] ? v[u][1] : 0.0f;
                in[2 * CS + at[u]] = ok[u] ? v[u][2] : 0.0f;
                in[3 * CS + at[u]] = ok[u] ? v[u][3] : 0.0f;
            }
        }
    }
    __syncthreads();
    float s[4][GF_OWN];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* pa = in + a * CS;
        gf_window_sums([=](int off) { return pa[off]; }, hs, r, RW, s[a]);
    }
#pragma unroll
    for (int k = 0; k < GF_OWN; ++k) {
        const int y = ty0 + 4 * (tid >> 5) + k, x = tx0 + (tid & 31);
        if (y >= H || x >= W) continue;
        const size_t pix = (size_t)y * W + x;
        const float* g = guide + pix * 3;
        const float N = (float)(gf_count(y, H, r) * gf_count(x, W, r));
        q[pix] = (s[0][k] / N) * g[0] + (s[1][k] / N) * g[1] + (s[2][k] / N) * g[2] + s[3][k] / N;
    }
}

AsrDeviceOnce g_prepare_lds, g_ab_lds, g_q_lds;

int gf_check_shape(const char* fn, int H, int W, int r) {
    ASR_REQUIRE(H >= 1 && W >= 1, "%s: bad shape H=%d W=%d", fn, H, W);
    ASR_REQUIRE(r >= 0, "%s: negative radius %d", fn, r);
    ASR_UNSUPPORTED(r > GF_RMAX, "%s: radius %d above the cap of %d (a 32 x 32 tile and its halo must fit a CU's LDS)", fn, r,
                    GF_RMAX);
    return ASR_OK;
}

}  // namespace

extern "C" size_t asr_guided_state_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return sizeof(float) * GF_STATE * (size_t)H * (size_t)W;
}

extern "C" size_t asr_guided_workspace_bytes(int planes, int H, int W) {
    if (planes < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * 4 * (size_t)planes * (size_t)H * (size_t)W;
}

extern "C" int asr_guided_prepare_f32(const float* guide, void* state, int H, int W, int r, float eps, asr_stream_t stream) {
    ASR_REQUIRE(guide && state, "asr_guided_prepare_f32: null pointer");
    const int rc = gf_check_shape("asr_guided_prepare_f32", H, W, r);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(isfinite(eps) && eps > 0.0f, "asr_guided_prepare_f32: eps must be finite and > 0 (got %g)", (double)eps);
    ASR_HIP_CHECK(asr_allow_dynamic_lds(g_prepare_lds, (const void*)guided_prepare_kernel, (int)gf_lds_bytes(3, GF_RMAX)));
    const dim3 grid((unsigned)asr_cdiv(W, GF_T), (unsigned)asr_cdiv(H, GF_T));
    hipLaunchKernelGGL(guided_prepare_kernel, grid, dim3(GF_THREADS), gf_lds_bytes(3, r), asr_stream(stream), guide,
                       (float*)state, H, W, r, eps);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_guided_apply_f32(const void* state, const float* guide, const float* p, float* q, void* workspace, int planes,
                                    int H, int W, int r, asr_stream_t stream) {
    ASR_REQUIRE(state && guide && p && q && workspace, "asr_guided_apply_f32: null pointer");
    ASR_REQUIRE(planes >= 1, "asr_guided_apply_f32: %d planes", planes);
    const int rc = gf_check_shape("asr_guided_apply_f32", H, W, r);
    if (rc != ASR_OK) return rc;
    ASR_UNSUPPORTED(planes > 65535, "asr_guided_apply_f32: %d planes above the cap of 65535 (a plane is a grid layer)", planes);
    ASR_HIP_CHECK(asr_allow_dynamic_lds(g_ab_lds, (const void*)guided_ab_kernel, (int)gf_lds_bytes(4, GF_RMAX)));
    ASR_HIP_CHECK(asr_allow_dynamic_lds(g_q_lds, (const void*)guided_q_kernel, (int)gf_lds_bytes(4, GF_RMAX)));
    const dim3 grid((unsigned)asr_cdiv(W, GF_T), (unsigned)asr_cdiv(H, GF_T), (unsigned)planes);
    hipLaunchKernelGGL(guided_ab_kernel, grid, dim3(GF_THREADS), gf_lds_bytes(4, r), asr_stream(stream), (const float*)state, guide,
                       p, (float*)workspace, H, W, r);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(guided_q_kernel, grid, dim3(GF_THREADS), gf_lds_bytes(4, r), asr_stream(stream), guide,
                       (const float*)workspace, q, H, W, r);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
