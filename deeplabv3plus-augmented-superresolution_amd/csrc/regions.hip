// Connected regions of label maps and the small-region clean-up built on them (include/asr_hip.h, "regions").
// Integer only: no floating point in this unit.
//
// asr_label_regions_i32, four launches on the caller's stream (no grid barrier, no flag, no workgroup waits for another):
//   rg_tile_kernel     one workgroup per RG_TW x RG_TH tile: union-find in LDS over the neighbour pairs INSIDE the tile (a pixel
//                      starts under the first pixel of its horizontal run; only the pairs nothing else implies are united), then
//                      parent[p] = the tile-local root's index in the map, count[p] = pixels of that root (0 elsewhere)
//   rg_merge_kernel    the neighbour pairs that straddle a tile border, same union routine on the parent plane in global memory
//   rg_flatten_kernel  root[p] = find(p), in place; a tile-local root that is not the region's root adds its count to the root's
//   rg_area_kernel     area[p] = count[root[p]]
// asr_clean_labels_i32: rg_surround_init_kernel, rg_surround_kernel (per-region min and max of the non-small neighbours' values),
// rg_relabel_kernel (the rule and the four statistics).
//
// Termination.  parent[i] <= i holds at every moment for every i: a plane starts at run starts (or, from the tile kernel, as
// the tile-local root, the smallest index of its tile component) and the only later writes are atomicMin(&parent[a], b) with
// b < a and the flatten's parent[p] = find(p) <= p.  A find step goes from i to parent[i] < i or ends, so a walk from p takes
// at most p < h*w steps.  A union step that does not end replaces the larger of its two indices by a smaller one, so the sum of
// the two falls every step: fewer than 2*h*w steps.  Both walks are counted loops with those caps; an overrun, which the
// invariant excludes, gives root = -1 (find: for that pixel; union: a flag word, and the flatten then writes -1 everywhere,
// since no labelling that a union gave up on can be trusted).
//
// Freshness.  Nothing here needs a load to return the latest value another workgroup wrote.  The values an address of the parent
// plane takes over time are a falling sequence of members of ONE set (a link only ever joins sets), so a stale parent is still a
// member of the same set with a smaller-or-equal index: walking from it reaches a root of the set all the same and only costs a
// step.  The one decision that must be exact -- "a was a root and now hangs under b" -- is taken from the value atomicMin
// RETURNS (old == a), never from a load.  Parents are read with relaxed agent-scope atomic loads all the same, so that a
// compiler never keeps one in a register across a step; kernel boundaries order the phases.
//
// Atomics per address.  Region sizes go through tile-local counts (LDS, one add per run of equal roots in a wave) and then ONE
// global add per tile-local root, so a map that is one region sends (tiles - 1) adds to its root's word, not h*w.  The surround
// min/max and the statistics are combined per wave (per run of equal roots) or per workgroup before they reach global memory.
#include "asr_common.h"
#include <limits.h>

namespace {

constexpr int RG_TW = ASR_REGIONS_TILE_W, RG_TH = ASR_REGIONS_TILE_H;
constexpr int RG_TILE = RG_TW * RG_TH;                    // 1024 pixels, four per thread
constexpr int RG_THREADS = 256;
constexpr int RG_OWN = RG_TILE / RG_THREADS;
static_assert(RG_TILE % RG_THREADS == 0 && RG_THREADS % 64 == 0 && (2 * 64) % RG_TW == 0, "tile / workgroup geometry");

#define RG_RELAXED_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define RG_RELAXED_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---- union-find, once on LDS (workgroup scope) and once on global memory (agent scope) -------------------------------------
// find: the root above i, or -1 after `cap` steps without reaching one (excluded by parent[i] <= i, see above)
template <bool LDS>
__device__ __forceinline__ int rg_find(int* parent, int i, unsigned cap) {
    for (unsigned n = 0; n <= cap; ++n) {
        const int q = LDS ? RG_RELAXED_WG(parent + i) : RG_RELAXED_AGENT(parent + i);
        if (q == i) return i;
        if (q < 0 || q > i) return -1;                     // never: keeps every index this walk forms inside [0, i]
        i = q;
    }
    return -1;
}

// union of the sets of a and b; false on an overrun
template <bool LDS>
__device__ __forceinline__ bool rg_union(int* parent, int a, int b, unsigned find_cap, unsigned cap) {
    for (unsigned n = 0; n <= cap; ++n) {
        a = rg_find<LDS>(parent, a, find_cap);
        b = rg_find<LDS>(parent, b, find_cap);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }      // a > b: hang a under b
        // only the returned value decides: old == a means a WAS a root at the instant of the link.  Otherwise a had a parent
        // old < a already; whichever of old and b the word keeps, the other still has to be joined: go on with (old, b).
        const int old = LDS ? __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                            : __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return true;
        if (old < 0 || old > a) return false;              // never (parent[a] <= a)
        a = old;
    }
    return false;
}

// ---- runs of equal keys over the consecutive lanes of a wave ----------------------------------------------------------------
__device__ __forceinline__ int rg_lane() { return (int)(threadIdx.x & 63u); }

// bit l set: lane l starts a run (its key differs from lane l - 1's).  Every lane of the wave must call this.
__device__ __forceinline__ unsigned long long rg_run_heads(int key) {
    const int lane = rg_lane();
    const int prev = __shfl_up(key, 1, 64);
    return __ballot(lane == 0 || prev != key);
}

// length of the run that starts at this (head) lane
__device__ __forceinline__ int rg_run_length(unsigned long long heads) {
    const int lane = rg_lane();
    const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    return (above ? __ffsll((long long)above) - 1 : 64) - lane;
}

// ---- (a) one tile in LDS ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_tile_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ parent_g,
                                                             int32_t* __restrict__ count_g, int* __restrict__ overrun, int h,
                                                             int w, int tiles_x, int c8) {
    __shared__ int lab[RG_TILE], par[RG_TILE], cnt[RG_TILE];
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * RG_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * RG_TH;
    const size_t plane = (size_t)blockIdx.y * ((size_t)h * (size_t)w);
    labels += plane; parent_g += plane; count_g += plane;
    bool ok[RG_OWN];
#pragma unroll
    for (int k = 0; k < RG_OWN; ++k) {
        const int i = tid + k * RG_THREADS;
        ok[k] = i % RG_TW < w - x0 && i / RG_TW < h - y0;     // (x0 + lx itself may pass 2^31 - 1 in a one-row map)
        const int v = ok[k] ? labels[(size_t)(y0 + i / RG_TW) * w + (x0 + i % RG_TW)] : 0;
        lab[i] = v;
        // The horizontal pairs cost no union: a wave holds two tile rows, and a pixel starts under the first pixel of its run
        // of equal values in its row (the highest run start at or below its lane; lanes 0 and 32 always start one).
        const int lane = rg_lane(), prev = __shfl_up(v, 1, 64);
        const unsigned long long starts = __ballot(i % RG_TW == 0 || !ok[k] || prev != v);
        const unsigned long long below = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        par[i] = i - (lane - (63 - __clzll((long long)below)));
        cnt[i] = 0;
    }
    __syncthreads();
    // The remaining pairs, each only where no other pair already implies it (every horizontal pair is joined):
    //   up         unless left and up-left are equal too: then left's own upward pair (or the one it defers to, further
    //              left; the chain ends at the first pixel of the overlap) joins the same two runs;
    //   up-left    only if neither up nor left is equal: up joins through (up, up-left), left through its own upward pair;
    //   up-right   only if up is not equal: up joins through (up, up-right).
    // A tile of one value makes 31 unions, not 2 * 1024.
    bool fine = true;
#pragma unroll
    for (int k = 0; k < RG_OWN; ++k) {
        const int i = tid + k * RG_THREADS, lx = i % RG_TW, ly = i / RG_TW;
        if (!ok[k] || ly == 0) continue;                     // a pixel inside the image has its left and upper neighbours inside too
        const int v = lab[i];
        const bool up = lab[i - RG_TW] == v, left = lx > 0 && lab[i - 1] == v, up_left = lx > 0 && lab[i - RG_TW - 1] == v;
        if (up && !(left && up_left)) fine &= rg_union<true>(par, i, i - RG_TW, RG_TILE, 2 * RG_TILE);
        if (c8) {
            if (up_left && !up && !left) fine &= rg_union<true>(par, i, i - RG_TW - 1, RG_TILE, 2 * RG_TILE);
            if (!up && lx < RG_TW - 1 && lx + 1 < w - x0 && lab[i - RG_TW + 1] == v)
                fine &= rg_union<true>(par, i, i - RG_TW + 1, RG_TILE, 2 * RG_TILE);
        }
    }
    __syncthreads();
    int r[RG_OWN];
#pragma unroll
    for (int k = 0; k < RG_OWN; ++k) {
        r[k] = ok[k] ? rg_find<true>(par, tid + k * RG_THREADS, RG_TILE) : -1;
        fine &= !ok[k] || r[k] >= 0;
    }
    // tile-local pixel counts: one LDS add per run of equal roots in the wave (a tile of one region: 16 adds, not 1024)
#pragma unroll
    for (int k = 0; k < RG_OWN; ++k) {
        const unsigned long long heads = rg_run_heads(r[k]);
        if (((heads >> rg_lane()) & 1ull) && r[k] >= 0) atomicAdd(&cnt[r[k]], rg_run_length(heads));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RG_OWN; ++k) {
        if (!ok[k]) continue;
        const int i = tid + k * RG_THREADS;
        const size_t p = (size_t)(y0 + i / RG_TW) * w + (x0 + i % RG_TW);
        // an overrun leaves the pixel its own parent: every index stays valid, and the flag makes the flatten write -1
        const int root = r[k] >= 0 ? r[k] : i;
        parent_g[p] = (int32_t)((size_t)(y0 + root / RG_TW) * w + (x0 + root % RG_TW));
        count_g[p] = root == i ? (r[k] >= 0 ? cnt[i] : 1) : 0;
    }
    if (!fine) atomicOr(overrun, 1);
}

// ---- (b) the neighbour pairs that straddle a tile border --------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_merge_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ parent,
                                                              int* __restrict__ overrun, int h, int w, int c8) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    if (pu >= n) return;
    const int p = (int)pu, x = p % w, y = p / w, lx = x % RG_TW, ly = y % RG_TH;
    if (lx != 0 && ly != 0 && lx != RG_TW - 1) return;      // all four backward neighbours share the pixel's tile
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    labels += plane; parent += plane;
    const int v = labels[p];
    const unsigned cap = 2u * n;
    bool fine = true;
    // The tile kernel's rules, which hold for the map as a whole: every horizontal pair is joined (inside a tile by the run
    // starts, across a border here, always), an upward pair defers to its left neighbour's where that one exists (same row, so
    // it is a pair of this kernel too), and a diagonal pair is joined only where no two joined 4-pairs imply it.  A map of one
    // value joins one upward pair per tile.
    const bool left = x > 0 && labels[p - 1] == v, up = y > 0 && labels[p - w] == v;
    const bool up_left = x > 0 && y > 0 && labels[p - w - 1] == v;
    if (lx == 0 && left) fine &= rg_union<false>(parent, p, p - 1, n, cap);
    if (ly == 0 && up && !(left && up_left)) fine &= rg_union<false>(parent, p, p - w, n, cap);
    if (c8 && y > 0) {
        if ((lx == 0 || ly == 0) && up_left && !up && !left) fine &= rg_union<false>(parent, p, p - w - 1, n, cap);
        if ((lx == RG_TW - 1 || ly == 0) && !up && x + 1 < w && labels[p - w + 1] == v)
            fine &= rg_union<false>(parent, p, p - w + 1, n, cap);
    }
    if (!fine) atomicOr(overrun, 1);
}

// ---- (c) + (d) flatten, and the tile-local counts to their roots ------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_flatten_kernel(int32_t* __restrict__ root, int32_t* __restrict__ count,
                                                                const int* __restrict__ overrun, int h, int w) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    if (pu >= n) return;
    const int p = (int)pu;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    root += plane; count += plane;
    // in place: root[p] = r is one more write that keeps parent[p] <= p inside p's set, so the walks of other threads through
    // p stay correct whichever value they see
    const int r = *overrun ? -1 : rg_find<false>(root, p, n);
    __hip_atomic_store(root + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // count[p] > 0 marks a tile-local root and is written by nobody but the tile kernel unless p is the region's root: only
    // the words of region roots receive adds, and their own threads (r == p) do not read them
    if (r >= 0 && r != p) {
        const int c = count[p];
        if (c > 0) atomicAdd(&count[r], c);
    }
}

__global__ __launch_bounds__(RG_THREADS) void rg_area_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ count,
                                                             int32_t* __restrict__ area, int h, int w) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    if (pu >= n) return;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    const int r = root[plane + pu];
    area[plane + pu] = r >= 0 ? count[plane + (unsigned)r] : 0;
}

// ---- clean-up ---------------------------------------------------------------------------------------------------------------
// vmin > vmax (INT_MAX, INT_MIN) is "no value yet"; one value v gives vmin == vmax == v; two different values vmin < vmax
__global__ __launch_bounds__(RG_THREADS) void rg_surround_init_kernel(int32_t* __restrict__ vmin, int32_t* __restrict__ vmax,
                                                                      int h, int w) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    if (pu >= n) return;
    const size_t i = (size_t)blockIdx.y * (size_t)n + pu;
    vmin[i] = INT_MAX; vmax[i] = INT_MIN;
}

// a root the kernels may index with: clean_labels takes root and area from its caller
__device__ __forceinline__ bool rg_root_ok(int r, unsigned n) { return r >= 0 && (unsigned)r < n; }

__global__ __launch_bounds__(RG_THREADS) void rg_surround_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ root,
                                                                 const int32_t* __restrict__ area, int32_t* __restrict__ vmin,
                                                                 int32_t* __restrict__ vmax, int h, int w, int c8, int min_area) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    labels += plane; root += plane; area += plane; vmin += plane; vmax += plane;
    // no early return: every lane takes part in the wave's shuffles below
    int key = -1, mn = INT_MAX, mx = INT_MIN;
    if (pu < n) {
        const int p = (int)pu, r = root[p];
        if (area[p] < min_area && rg_root_ok(r, n)) {
            key = r;
            const int x = p % w, y = p / w;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                constexpr int DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};
                if (d >= 4 && !c8) break;
                const int qx = x + DX[d], qy = y + DY[d];
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const int q = qy * w + qx;
                if (root[q] == r || area[q] < min_area) continue;          // inside R, or a small region: never votes
                const int v = labels[q];
                mn = min(mn, v); mx = max(mx, v);
            }
        }
    }
    // min and max over each run of equal roots in the wave, then one pair of atomics per run that saw a value.  A run id, not
    // the root, bounds the combination, though min and max would forgive a lane counted twice.
    const int lane = rg_lane();
    const unsigned long long heads = rg_run_heads(key);
    const int rid = __popcll(heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int omn = __shfl_down(mn, o, 64), omx = __shfl_down(mx, o, 64), orid = __shfl_down(rid, o, 64);
        if (lane + o < 64 && orid == rid) { mn = min(mn, omn); mx = max(mx, omx); }
    }
    if (((heads >> lane) & 1ull) && key >= 0 && mn <= mx) {
        atomicMin(&vmin[key], mn);
        atomicMax(&vmax[key], mx);
    }
}

__global__ __launch_bounds__(RG_THREADS) void rg_relabel_kernel(const int32_t* labels, const int32_t* __restrict__ root,
                                                                const int32_t* __restrict__ area, const int32_t* __restrict__ vmin,
                                                                const int32_t* __restrict__ vmax, int32_t* out,
                                                                unsigned long long* __restrict__ stats, int h, int w, int min_area) {
    __shared__ unsigned int part[RG_THREADS / 64][4];
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned pu = blockIdx.x * (unsigned)RG_THREADS + threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * (size_t)n;
    unsigned int s[4] = {0u, 0u, 0u, 0u};                    // regions, small regions, pixels in small regions, pixels changed
    if (pu < n) {
        const int p = (int)pu, r = root[plane + pu], v = labels[plane + pu];
        const bool small = area[plane + pu] < min_area;
        int o = v;
        if (small && rg_root_ok(r, n)) {
            const int a = vmin[plane + (unsigned)r], b = vmax[plane + (unsigned)r];
            o = a == b ? a : 0;
        }
        out[plane + pu] = o;                                  // out may be labels: this thread alone reads and writes the word
        s[0] = r == p; s[1] = r == p && small; s[2] = small; s[3] = o != v;
    }
    if (!stats) return;                                       // uniform over the grid
    const int lane = rg_lane(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
        if (lane == 0) part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned int t = 0;
        for (int v = 0; v < RG_THREADS / 64; ++v) t += part[v][threadIdx.x];
        if (t) atomicAdd(&stats[4 * (size_t)blockIdx.y + threadIdx.x], (unsigned long long)t);
    }
}

int rg_check_shape(const char* fn, int maps, int h, int w, int connectivity) {
    ASR_REQUIRE(h >= 1 && w >= 1, "%s: bad shape h=%d w=%d", fn, h, w);
    ASR_REQUIRE((int64_t)h * (int64_t)w <= (int64_t)INT_MAX, "%s: h*w = %lld above 2^31 - 1 (roots are int32 indices)", fn,
                (long long)h * (long long)w);
    ASR_REQUIRE(maps >= 1 && maps <= 65535, "%s: %d maps (1..65535: a map is a grid layer)", fn, maps);
    ASR_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d (4 or 8)", fn, connectivity);
    return ASR_OK;
}

size_t rg_cells(int maps, int h, int w) { return (size_t)maps * (size_t)h * (size_t)w; }

}  // namespace

// the tile-local counts [maps, h, w] int32 and, 8-byte aligned behind them, the overrun word
extern "C" size_t asr_label_regions_workspace_bytes(int maps, int h, int w) {
    if (maps < 1 || h < 1 || w < 1) return 0;
    return (rg_cells(maps, h, w) * sizeof(int32_t) + 7) / 8 * 8 + 8;
}

extern "C" int asr_label_regions_i32(const int32_t* labels, int32_t* root, int32_t* area, void* workspace, size_t workspace_bytes,
                                     int maps, int h, int w, int connectivity, asr_stream_t stream) {
    ASR_REQUIRE(labels && root && area && workspace, "asr_label_regions_i32: null pointer");
    const int rc = rg_check_shape("asr_label_regions_i32", maps, h, w, connectivity);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "asr_label_regions_i32: workspace not aligned to 4 bytes");
    const size_t need = asr_label_regions_workspace_bytes(maps, h, w);
    if (workspace_bytes < need) {
        asr_set_error("asr_label_regions_i32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    int32_t* count = (int32_t*)workspace;
    int* overrun = (int*)((char*)workspace + need - 8);
    const int tiles_x = (int)asr_cdiv(w, RG_TW), c8 = connectivity == 8;
    const int64_t tiles = (int64_t)tiles_x * asr_cdiv(h, RG_TH);        // < 2^31: h*w < 2^31 and at least one pixel per tile
    const dim3 pixels((unsigned)asr_cdiv((int64_t)h * w, RG_THREADS), (unsigned)maps);
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(overrun, 0, sizeof(int), s));
    hipLaunchKernelGGL(rg_tile_kernel, dim3((unsigned)tiles, (unsigned)maps), dim3(RG_THREADS), 0, s, labels, root, count, overrun, h,
                       w, tiles_x, c8);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_merge_kernel, pixels, dim3(RG_THREADS), 0, s, labels, root, overrun, h, w, c8);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_flatten_kernel, pixels, dim3(RG_THREADS), 0, s, root, count, (const int*)overrun, h, w);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_area_kernel, pixels, dim3(RG_THREADS), 0, s, (const int32_t*)root, (const int32_t*)count, area, h, w);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// the surround's two planes [maps, h, w] int32: minimum and maximum of the non-small neighbours' values, indexed by root
extern "C" size_t asr_clean_labels_workspace_bytes(int maps, int h, int w) {
    if (maps < 1 || h < 1 || w < 1) return 0;
    return 2 * rg_cells(maps, h, w) * sizeof(int32_t);
}

extern "C" int asr_clean_labels_i32(const int32_t* labels, const int32_t* root, const int32_t* area, int32_t* out, int64_t* stats,
                                    void* workspace, size_t workspace_bytes, int maps, int h, int w, int connectivity, int min_area,
                                    asr_stream_t stream) {
    ASR_REQUIRE(labels && root && area && out && workspace, "asr_clean_labels_i32: null pointer");
    const int rc = rg_check_shape("asr_clean_labels_i32", maps, h, w, connectivity);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(min_area >= 1, "asr_clean_labels_i32: min_area %d below 1", min_area);
    ASR_REQUIRE(((uintptr_t)workspace & 3u) == 0, "asr_clean_labels_i32: workspace not aligned to 4 bytes");
    ASR_REQUIRE(((uintptr_t)stats & 7u) == 0, "asr_clean_labels_i32: stats not aligned to 8 bytes");
    const size_t need = asr_clean_labels_workspace_bytes(maps, h, w);
    if (workspace_bytes < need) {
        asr_set_error("asr_clean_labels_i32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    const size_t cells = rg_cells(maps, h, w);
    int32_t *vmin = (int32_t*)workspace, *vmax = vmin + cells;
    const dim3 pixels((unsigned)asr_cdiv((int64_t)h * w, RG_THREADS), (unsigned)maps);
    hipStream_t s = asr_stream(stream);
    if (stats) ASR_HIP_CHECK(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t) * (size_t)maps, s));
    hipLaunchKernelGGL(rg_surround_init_kernel, pixels, dim3(RG_THREADS), 0, s, vmin, vmax, h, w);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_surround_kernel, pixels, dim3(RG_THREADS), 0, s, labels, root, area, vmin, vmax, h, w,
                       (int)(connectivity == 8), min_area);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_relabel_kernel, pixels, dim3(RG_THREADS), 0, s, labels, root, area, (const int32_t*)vmin,
                       (const int32_t*)vmax, out, (unsigned long long*)stats, h, w, min_area);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
