// Label maps scored region by region: the regions of a prediction matched against the regions of the truth
// (include/asr_hip.h, "segments").  Integer only: no floating point in this unit.
//
// asr_segment_match_i32, three memsets and four launches on the caller's stream (no grid barrier, no flag, no workgroup waits
// for another; a kernel boundary is the only ordering relied on):
//   sg_pairs_kernel   one workgroup per SG_TW x SG_TH tile: the tile's distinct (truth root, predicted root) pairs and their pixel
//                     counts gathered in an open-addressed LDS table (2048 slots for at most 1024 pairs), then every distinct pair
//                     added ONCE to the map's global table: the 64-bit key claimed by compare-and-swap, the count by an atomic add
//   sg_area_kernel    walks the table: A_p[predicted root] += count (void pixels never entered the table)
//   sg_match_kernel   walks the table: equal segment values and 3 I > A_g + A_p make a match; it notes each side's partner at
//                     the two roots and adds TP and floor(I 2^30 / union), summed per workgroup in LDS first
//   sg_finish_kernel  walks the pixels: a pixel that is its own root and has no partner is an FN (truth) or, unless dropped, an
//                     FP (prediction), summed per workgroup in LDS first; writes the two optional planes
//
// The pairs that enter the table are those of the pixels whose predicted value is a segment value and whose truth is not void:
// exactly the pixels A_p and every I count.  A map has at most h*w of them and the table at least 2*h*w slots, so a probe
// sequence always meets its key or a free slot: there is no overflow path.  Every probe sequence is a counted loop all the same.
//
// A root that is not an index of the map (the planes come from the caller) makes its pixel take no part, so no index formed
// here leaves [0, h*w).
#include "asr_common.h"
#include <limits.h>

namespace {

constexpr int SG_TW = ASR_REGIONS_TILE_W, SG_TH = ASR_REGIONS_TILE_H;
constexpr int SG_TILE = SG_TW * SG_TH;                     // 1024 pixels, four per thread
constexpr int SG_THREADS = 256;
constexpr int SG_OWN = SG_TILE / SG_THREADS;
constexpr int SG_SLOTS = 2 * SG_TILE;                      // the LDS table: never more than half full
constexpr int SG_L = ASR_SEGMENTS_MAX_LABELS;
constexpr unsigned long long SG_EMPTY = ~0ull;             // no pair: a root is never negative
static_assert(SG_TILE % SG_THREADS == 0 && SG_SLOTS % SG_THREADS == 0 && (SG_SLOTS & (SG_SLOTS - 1)) == 0, "tile / table geometry");

typedef unsigned long long sg_u64;

__device__ __forceinline__ sg_u64 sg_key(int truth_root, int pred_root) {
    return ((sg_u64)(unsigned)truth_root << 32) | (sg_u64)(unsigned)pred_root;
}

// the 64-bit finaliser of MurmurHash3: every input bit reaches every output bit
__device__ __forceinline__ sg_u64 sg_hash(sg_u64 k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

__device__ __forceinline__ bool sg_root_ok(int r, unsigned n) { return r >= 0 && (unsigned)r < n; }
__device__ __forceinline__ bool sg_is_segment(int v, int v0, int L) { return v >= v0 && v < L; }

__device__ __forceinline__ int sg_lane() { return (int)(threadIdx.x & 63u); }

// ---- (a) a tile's distinct pairs in LDS, then each once to the global table ------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_pairs_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ truth_root,
                                                              const int32_t* __restrict__ preds, const int32_t* __restrict__ pred_root,
                                                              sg_u64* __restrict__ keys_g, unsigned* __restrict__ cnt_g,
                                                              sg_u64 cap, int h, int w, int tiles_x, int L, int v0) {
    __shared__ sg_u64 key_s[SG_SLOTS];
    __shared__ unsigned cnt_s[SG_SLOTS];
    const int tid = threadIdx.x;
    const unsigned n = (unsigned)h * (unsigned)w;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * SG_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * SG_TH;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    preds += plane; pred_root += plane;
    keys_g += (size_t)blockIdx.y * cap; cnt_g += (size_t)blockIdx.y * cap;
    for (int s = tid; s < SG_SLOTS; s += SG_THREADS) { key_s[s] = SG_EMPTY; cnt_s[s] = 0u; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SG_OWN; ++k) {
        const int i = tid + k * SG_THREADS;
        sg_u64 key = SG_EMPTY;
        if (i % SG_TW < w - x0 && i / SG_TW < h - y0) {      // (x0 + lx itself may pass 2^31 - 1 in a one-row map)
            const size_t p = (size_t)(y0 + i / SG_TW) * w + (x0 + i % SG_TW);
            const int t = truth[p], v = preds[p], tr = truth_root[p], pr = pred_root[p];
            if (t >= 0 && t < L && sg_is_segment(v, v0, L) && sg_root_ok(tr, n) && sg_root_ok(pr, n)) key = sg_key(tr, pr);
        }
        // one LDS add per run of equal pairs over the consecutive lanes of the wave (two tile rows); no early exit above: every
        // lane takes part in the shuffles
        const int lane = sg_lane();
        const unsigned lo = __shfl_up((unsigned)key, 1, 64), hi = __shfl_up((unsigned)(key >> 32), 1, 64);
        const sg_u64 heads = __ballot(lane == 0 || (((sg_u64)hi << 32) | lo) != key);
        if (((heads >> lane) & 1ull) && key != SG_EMPTY) {
            const sg_u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
            const unsigned run = (unsigned)((above ? __ffsll((long long)above) - 1 : 64) - lane);
            unsigned s = (unsigned)sg_hash(key) & (SG_SLOTS - 1);
            for (int probe = 0; probe < SG_SLOTS; ++probe) {
                sg_u64 seen = SG_EMPTY;
                if (__hip_atomic_compare_exchange_strong(&key_s[s], &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP) || seen == key) {
                    __hip_atomic_fetch_add(&cnt_s[s], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                s = (s + 1u) & (SG_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    const sg_u64 mask = cap - 1ull;
    for (int s = tid; s < SG_SLOTS; s += SG_THREADS) {
        const sg_u64 key = key_s[s];
        if (key == SG_EMPTY) continue;
        const unsigned c = cnt_s[s];
        sg_u64 g = (sg_hash(key) >> 11) & mask;              // other bits than the LDS table took
        for (sg_u64 probe = 0; probe < cap; ++probe) {
            sg_u64 seen = SG_EMPTY;
            if (__hip_atomic_compare_exchange_strong(&keys_g[g], &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT) || seen == key) {
                __hip_atomic_fetch_add(&cnt_g[g], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            g = (g + 1ull) & mask;
        }
    }
}

// ---- (b) A_p: a predicted segment's pixels where the truth is not void ------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_area_kernel(const sg_u64* __restrict__ keys_g, const unsigned* __restrict__ cnt_g,
                                                             int32_t* __restrict__ pred_area, sg_u64 cap, unsigned n) {
    const sg_u64 g = (sg_u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (g >= cap) return;
    const sg_u64 key = keys_g[(size_t)blockIdx.y * cap + g];
    if (key == SG_EMPTY) return;
    const unsigned pr = (unsigned)key;
    if (pr >= n) return;                                      // never: the pairs kernel checked it
    __hip_atomic_fetch_add(&pred_area[(size_t)blockIdx.y * n + pr], (int)cnt_g[(size_t)blockIdx.y * cap + g], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// ---- (c) the matches --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_match_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ truth_area,
                                                              const int32_t* __restrict__ preds, const sg_u64* __restrict__ keys_g,
                                                              const unsigned* __restrict__ cnt_g, const int32_t* __restrict__ pred_area,
                                                              int32_t* __restrict__ truth_partner, int32_t* __restrict__ pred_partner,
                                                              sg_u64* __restrict__ counts, sg_u64 cap, unsigned n, int L, int v0) {
    __shared__ unsigned tp_s[SG_L];
    __shared__ sg_u64 q_s[SG_L];
    if (threadIdx.x < SG_L) { tp_s[threadIdx.x] = 0u; q_s[threadIdx.x] = 0ull; }
    __syncthreads();
    const sg_u64 g = (sg_u64)blockIdx.x * SG_THREADS + threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    if (g < cap) {
        const sg_u64 key = keys_g[(size_t)blockIdx.y * cap + g];
        const unsigned tr = (unsigned)(key >> 32), pr = (unsigned)key;
        if (key != SG_EMPTY && tr < n && pr < n) {
            const int v = truth[tr];
            if (sg_is_segment(v, v0, L) && preds[plane + pr] == v) {
                const long long inter = (long long)cnt_g[(size_t)blockIdx.y * cap + g];
                const long long both = (long long)truth_area[tr] + (long long)pred_area[plane + pr];
                // IoU > 1/2, strictly.  both - inter > 0 then: inter <= min(A_g, A_p) would make 3 inter <= both otherwise
                if (3 * inter > both && both - inter > 0) {
                    truth_partner[plane + tr] = (int32_t)pr;  // the one match of either segment: no other thread writes these
                    pred_partner[plane + pr] = (int32_t)tr;
                    const sg_u64 q = (sg_u64)((inter << 30) / (both - inter));
                    __hip_atomic_fetch_add(&tp_s[v], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&q_s[v], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < L && tp_s[threadIdx.x]) {
        sg_u64* c = counts + ((size_t)blockIdx.y * L + threadIdx.x) * 4;
        __hip_atomic_fetch_add(c + 0, (sg_u64)tp_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(c + 3, q_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- (d) FN and FP from the pixels that are their own root, and the two planes ----------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_finish_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ truth_root,
                                                               const int32_t* __restrict__ preds, const int32_t* __restrict__ pred_root,
                                                               const int32_t* __restrict__ pred_area,
                                                               const int32_t* __restrict__ truth_partner,
                                                               const int32_t* __restrict__ pred_partner, sg_u64* __restrict__ counts,
                                                               int32_t* __restrict__ pred_match, int32_t* __restrict__ truth_match,
                                                               unsigned n, int L, int v0) {
    __shared__ unsigned fp_s[SG_L], fn_s[SG_L];
    if (threadIdx.x < SG_L) { fp_s[threadIdx.x] = 0u; fn_s[threadIdx.x] = 0u; }
    __syncthreads();
    const unsigned pu = blockIdx.x * (unsigned)SG_THREADS + threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    if (pu < n) {
        const int t = truth[pu], tr = truth_root[pu];
        int tm = -2;
        if (sg_is_segment(t, v0, L) && sg_root_ok(tr, n)) {
            tm = truth_partner[plane + (unsigned)tr];
            if ((unsigned)tr == pu && tm < 0) __hip_atomic_fetch_add(&fn_s[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (truth_match) truth_match[plane + pu] = tm;
        const int v = preds[plane + pu], pr = pred_root[plane + pu];
        int pm = -2;
        if (sg_is_segment(v, v0, L) && sg_root_ok(pr, n) && pred_area[plane + (unsigned)pr] > 0) {   // A_p = 0: dropped
            pm = pred_partner[plane + (unsigned)pr];
            if ((unsigned)pr == pu && pm < 0) __hip_atomic_fetch_add(&fp_s[v], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (pred_match) pred_match[plane + pu] = pm;
    }
    __syncthreads();
    if ((int)threadIdx.x < L) {
        sg_u64* c = counts + ((size_t)blockIdx.y * L + threadIdx.x) * 4;
        if (fp_s[threadIdx.x]) __hip_atomic_fetch_add(c + 1, (sg_u64)fp_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fn_s[threadIdx.x]) __hip_atomic_fetch_add(c + 2, (sg_u64)fn_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// slots of one map's table: the power of two at or above 2*h*w (h*w <= 2^31 - 1: at most 2^32)
sg_u64 sg_capacity(int h, int w) {
    const sg_u64 want = 2ull * (sg_u64)h * (sg_u64)w;
    sg_u64 cap = 2;
    while (cap < want) cap <<= 1;
    return cap;
}

}  // namespace

// Per map: the table's keys [cap] u64, the two partner planes [h, w] int32 (all three start as all-ones bytes: no pair, -1),
// then the table's counts [cap] u32 and A_p [h, w] int32 (both start as zero).
extern "C" size_t asr_segment_match_workspace_bytes(int maps, int h, int w) {
    if (maps < 1 || h < 1 || w < 1) return 0;
    return (size_t)maps * ((size_t)sg_capacity(h, w) * 12 + (size_t)h * (size_t)w * 12);
}

extern "C" int asr_segment_match_i32(const int32_t* truth, const int32_t* truth_root, const int32_t* truth_area,
                                     const int32_t* preds, const int32_t* pred_root, int64_t* counts, int32_t* pred_match,
                                     int32_t* truth_match, void* workspace, size_t workspace_bytes, int maps, int h, int w,
                                     int num_labels, int include_zero, asr_stream_t stream) {
    ASR_REQUIRE(truth && truth_root && truth_area && preds && pred_root && counts && workspace,
                "asr_segment_match_i32: null pointer");
    ASR_REQUIRE(num_labels >= 1 && num_labels <= ASR_SEGMENTS_MAX_LABELS, "asr_segment_match_i32: %d labels (1..%d)", num_labels,
                ASR_SEGMENTS_MAX_LABELS);
    ASR_REQUIRE(h >= 1 && w >= 1, "asr_segment_match_i32: bad shape h=%d w=%d", h, w);
    ASR_REQUIRE((int64_t)h * (int64_t)w <= (int64_t)INT_MAX, "asr_segment_match_i32: h*w = %lld above 2^31 - 1 (roots are int32 indices)",
                (long long)h * (long long)w);
    ASR_REQUIRE(maps >= 1 && maps <= 65535, "asr_segment_match_i32: %d maps (1..65535: a map is a grid layer)", maps);
    ASR_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)counts & 7u) == 0,
                "asr_segment_match_i32: workspace and counts must be aligned to 8 bytes");
    const size_t need = asr_segment_match_workspace_bytes(maps, h, w);
    if (workspace_bytes < need) {
        asr_set_error("asr_segment_match_i32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    const sg_u64 cap = sg_capacity(h, w);
    const unsigned n = (unsigned)h * (unsigned)w;
    const size_t slots = (size_t)maps * (size_t)cap, cells = (size_t)maps * (size_t)n;
    sg_u64* keys = (sg_u64*)workspace;
    int32_t* truth_partner = (int32_t*)(keys + slots);
    int32_t* pred_partner = truth_partner + cells;
    unsigned* cnt = (unsigned*)(pred_partner + cells);
    int32_t* pred_area = (int32_t*)(cnt + slots);
    const int tiles_x = (int)asr_cdiv(w, SG_TW), v0 = include_zero ? 0 : 1;
    const int64_t tiles = (int64_t)tiles_x * asr_cdiv(h, SG_TH);        // < 2^31: h*w < 2^31 and at least one pixel per tile
    const dim3 pixels((unsigned)asr_cdiv((int64_t)n, SG_THREADS), (unsigned)maps);
    const dim3 table((unsigned)asr_cdiv((int64_t)cap, SG_THREADS), (unsigned)maps);
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(keys, 0xFF, slots * 8 + cells * 8, s));
    ASR_HIP_CHECK(hipMemsetAsync(cnt, 0, slots * 4 + cells * 4, s));
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 4 * (size_t)num_labels * (size_t)maps, s));
    hipLaunchKernelGGL(sg_pairs_kernel, dim3((unsigned)tiles, (unsigned)maps), dim3(SG_THREADS), 0, s, truth, truth_root, preds,
                       pred_root, keys, cnt, cap, h, w, tiles_x, num_labels, v0);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_area_kernel, table, dim3(SG_THREADS), 0, s, (const sg_u64*)keys, (const unsigned*)cnt, pred_area, cap, n);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_match_kernel, table, dim3(SG_THREADS), 0, s, truth, truth_area, preds, (const sg_u64*)keys,
                       (const unsigned*)cnt, (const int32_t*)pred_area, truth_partner, pred_partner, (sg_u64*)counts, cap, n,
                       num_labels, v0);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_finish_kernel, pixels, dim3(SG_THREADS), 0, s, truth, truth_root, preds, pred_root,
                       (const int32_t*)pred_area, (const int32_t*)truth_partner, (const int32_t*)pred_partner, (sg_u64*)counts,
                       pred_match, truth_match, n, num_labels, v0);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
