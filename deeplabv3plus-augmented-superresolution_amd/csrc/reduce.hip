// Output-processing (OPM), thresholding and IoU counting kernels (gfx950).
//
// Reference (paths in /root/reference):
//   utils.py:115-119                                    create_mask (argmax)
//   superresolution_scripts/augmentation_utils.py:80-115  OPM modes argmax / slice / slice_max
//   superresolution_scripts/superres_utils.py:56-62,118-139  min_max_normalization, threshold_image
//   utils.py:180-204                                    single_class_IOU (integer counts)
// All of these are HBM-bound single passes; per-segment reductions use wave shuffles and one
// block per segment so the results are deterministic.
#include "asr_common.h"

namespace {

// ---- per-segment min / max ------------------------------------------------------------------
// A segment is split over several workgroups (a single 1024-thread workgroup per segment left 255 CUs idle on the
// one-segment calls of the hot path: 190 us for 1.6 M floats); partial results meet in out[] through integer atomics
// on the float bit patterns (min / max are order-independent, so the result is exact).
__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
    v += 0.0f;                                     // -0.0 -> +0.0: the sign test below must agree with the bit pattern
    if (v >= 0.0f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
    v += 0.0f;
    if (v >= 0.0f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

__global__ __launch_bounds__(256) void minmax_init_kernel(float* __restrict__ out, int segments) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < segments) { out[2 * i] = INFINITY; out[2 * i + 1] = -INFINITY; }
}

__global__ __launch_bounds__(1024) void minmax_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                      int64_t per_seg) {
    __shared__ float smin[16], smax[16];
    const float* p = x + (int64_t)blockIdx.y * per_seg;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 1024) {
        const float v = p[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = asr_wave_min(mn);
    mx = asr_wave_max(mx);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { smin[wave] = mn; smax[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) { mn = fminf(mn, smin[i]); mx = fmaxf(mx, smax[i]); }
        atomic_min_float(out + blockIdx.y * 2 + 0, mn);
        atomic_max_float(out + blockIdx.y * 2 + 1, mx);
    }
}

// ---- argmax over the class axis (first maximum wins, like tf.argmax) --------------------------
__device__ __forceinline__ int argmax_row(const float* __restrict__ row, int classes) {
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < classes; ++c) {
        const float v = row[c];
        if (v > best) { best = v; arg = c; }
    }
    return arg;
}

// The class rows are 4 * classes bytes apart (84 for 21 classes): a thread walking its own row makes every wave-load a
// 64-way strided gather that pulls whole cache lines for 4 bytes each (PMC: 7.3x the logits' bytes fetched).  A
// workgroup therefore copies its 256 consecutive rows into LDS with coalesced loads and the threads walk the LDS rows
// (stride of `classes` words: conflict-free for odd class counts such as 21).  kMaxStageClasses bounds the LDS tile.
constexpr int kMaxStageClasses = 32;

__device__ __forceinline__ float* stage_rows(const float* __restrict__ logits, int64_t first, int64_t pixels, int classes,
                                             float* __restrict__ tile) {
    const int64_t rows = min((int64_t)256, pixels - first);
    const int64_t n = rows * classes;
    const float* src = logits + first * classes;
    for (int64_t i = threadIdx.x; i < n; i += 256) tile[i] = src[i];
    __syncthreads();
    return tile + (int64_t)threadIdx.x * classes;
}

// STAGED: the rows go through LDS; else the same walk straight from global memory, for class counts beyond the LDS tile
template <bool STAGED>
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int32_t* __restrict__ out,
                                                     int64_t pixels, int classes) {
    __shared__ float tile[STAGED ? 256 * kMaxStageClasses : 1];
    for (int64_t first = (int64_t)blockIdx.x * 256; first < pixels; first += (int64_t)gridDim.x * 256) {
        const int64_t p = first + threadIdx.x;
        const float* row = STAGED ? stage_rows(logits, first, pixels, classes, tile) : logits + p * classes;
        if (p < pixels) out[p] = argmax_row(row, classes);
        if (STAGED) __syncthreads();
    }
}

// ---- OPM of a class set (asr_opm_classes_f32; asr_opm_argmax_f32 / _slice_f32 / _slice_max_f32 are its sets of one) ------
// Each pixel's row is read once -- through LDS like argmax_kernel when it fits (STAGED), else straight from global memory --
// and every class of the set gets the same statements on it: argmax_row once per pixel, then one compare per class
// (ARGMAX: the id where it wins, else 0); the class logit min-max normalised by its copy's global minimum / maximum
// seg_minmax[copy] (SLICE, one copy per grid row); the class logit and the maximum over the other classes, folded in class
// order, once per class (SLICE_MAX).  Plane k of the output lies class_stride floats after plane k-1.  argmax / slice_max
// launch one "copy" of all pixels.
template <int MODE, bool STAGED>
__global__ __launch_bounds__(256) void opm_classes_kernel(const float* __restrict__ logits, float* __restrict__ cls,
                                                          float* __restrict__ mx, const float* __restrict__ seg_minmax,
                                                          int64_t per_copy, int classes, int64_t class_stride, AsrClassSet set,
                                                          float new_min, float new_max) {
    __shared__ float tile[STAGED ? 256 * kMaxStageClasses : 1];
    const int copy = blockIdx.y;
    const float* base = logits + (int64_t)copy * per_copy * classes;
    const int64_t o0 = (int64_t)copy * per_copy;
    float mn = 0.0f, den = 1.0f, span = 0.0f;
    if (MODE == ASR_OPM_SLICE) {
        mn = seg_minmax[copy * 2 + 0];
        const float mxv = seg_minmax[copy * 2 + 1];
        den = ((mxv - mn) != 0.0f) ? (mxv - mn) : 1.0f;
        span = new_max - new_min;
    }
    for (int64_t first = (int64_t)blockIdx.x * 256; first < per_copy; first += (int64_t)gridDim.x * 256) {
        const int64_t p = first + threadIdx.x;
        const float* row = STAGED ? stage_rows(base, first, per_copy, classes, tile) : base + p * classes;
        if (p < per_copy) {
            float* c = cls + o0 + p;
            if (MODE == ASR_OPM_ARGMAX) {
                const int arg = argmax_row(row, classes);
                for (int k = 0; k < set.n; ++k) c[k * class_stride] = (arg == set.id[k]) ? (float)set.id[k] : 0.0f;
            } else if (MODE == ASR_OPM_SLICE) {
                for (int k = 0; k < set.n; ++k) {
                    const float num = (row[set.id[k]] - mn) * span;
                    c[k * class_stride] = new_min + num / den;
                }
            } else {
                float* m = mx + o0 + p;
                for (int k = 0; k < set.n; ++k) {
                    const int id = set.id[k];
                    float best = -INFINITY;
                    for (int j = 0; j < classes; ++j)
                        if (j != id) best = fmaxf(best, row[j]);
                    c[k * class_stride] = row[id];
                    m[k * class_stride] = best;
                }
            }
        }
        if (STAGED) __syncthreads();
    }
}

// ---- min_max_normalization of a stack with its own global minimum / maximum (load_SR_data, superres_utils.py:183-206) ----
__global__ __launch_bounds__(256) void minmax_normalize_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                               const float* __restrict__ seg_minmax, int64_t per_seg,
                                                               float new_min, float new_max) {
    const int seg = blockIdx.y;
    const float mn = seg_minmax[seg * 2 + 0], mxv = seg_minmax[seg * 2 + 1];
    const float den = ((mxv - mn) != 0.0f) ? (mxv - mn) : 1.0f;
    const float span = new_max - new_min;
    const float* p = x + (int64_t)seg * per_seg;
    float* o = out + (int64_t)seg * per_seg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 256)
        o[i] = new_min + ((p[i] - mn) * span) / den;
}

// ---- threshold_image -----------------------------------------------------------------------------
__device__ __forceinline__ void threshold_segment(const float* __restrict__ img, const float* __restrict__ th_mask,
                                                  const float* __restrict__ seg_minmax, int32_t* __restrict__ out,
                                                  int64_t per_seg, float th_factor, int th_value, int seg) {
    const float* p = img + (int64_t)seg * per_seg;
    int32_t* o = out + (int64_t)seg * per_seg;
    if (th_mask) {
        const float* t = th_mask + (int64_t)seg * per_seg;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 256)
            o[i] = (p[i] >= t[i]) ? th_value : 0;
    } else {
        const float th = seg_minmax[seg * 2 + 1] * th_factor;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 256)
            o[i] = (p[i] > th) ? th_value : 0;
    }
}

__global__ __launch_bounds__(256) void threshold_kernel(const float* __restrict__ img, const float* __restrict__ th_mask,
                                                        const float* __restrict__ seg_minmax, int32_t* __restrict__ out,
                                                        int64_t per_seg, float th_factor, int th_value) {
    threshold_segment(img, th_mask, seg_minmax, out, per_seg, th_factor, th_value, blockIdx.y);
}

// segment k is thresholded to values.id[k] (asr_threshold_classes_f32)
__global__ __launch_bounds__(256) void threshold_classes_kernel(const float* __restrict__ img, const float* __restrict__ th_mask,
                                                                const float* __restrict__ seg_minmax, int32_t* __restrict__ out,
                                                                int64_t per_seg, float th_factor, AsrClassSet values) {
    threshold_segment(img, th_mask, seg_minmax, out, per_seg, th_factor, values.id[blockIdx.y], blockIdx.y);
}

// ---- IoU counts: counts[seg] = {inter_c, union_c, inter_bg, union_bg} ------------------------------
__global__ __launch_bounds__(256) void iou_counts_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ pred,
                                                         unsigned long long* __restrict__ counts, int64_t per_seg,
                                                         int64_t truth_stride, int class_id, int include_bg) {
    const int seg = blockIdx.y;
    const int32_t* t = truth + (int64_t)seg * truth_stride;          // truth_stride 0: every segment against one label map
    const int32_t* q = pred + (int64_t)seg * per_seg;
    unsigned int ic = 0, uc = 0, ib = 0, ub = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 256) {
        int tv = t[i];
        const int pv = q[i];
        if (include_bg && tv != class_id) tv = 0;  // utils.py:188-190
        const bool tc = tv == class_id, pc = pv == class_id;
        ic += (tc && pc); uc += (tc || pc);
        const bool tb = tv == 0, pb = pv == 0;
        ib += (tb && pb); ub += (tb || pb);
    }
    auto wsum = [](unsigned int v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
    };
    ic = wsum(ic); uc = wsum(uc); ib = wsum(ib); ub = wsum(ub);
    // one set of 64-bit atomics per workgroup (per-wave atomics on four shared addresses serialised the launch)
    __shared__ unsigned int part[4][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = ic; part[wave][1] = uc; part[wave][2] = ib; part[wave][3] = ub; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                     part[3][threadIdx.x];
        if (v) atomicAdd(counts + seg * 4 + threadIdx.x, v);
    }
}

// ---- IoU counts of a class set: K classes x M masks against one label map, in one pass over it ---------------------
// Each thread loads its truth pixel once; for every (class k, mask m) a wave counts the four predicates of iou_counts_kernel
// by ballot and its lane 0 adds them to the wave's own LDS row (no atomics inside the workgroup).  Out-of-range lanes take
// part in the ballots with every predicate false: the trip count is uniform over the workgroup.
constexpr int kMaxIouMasks = 8;

__global__ __launch_bounds__(256) void iou_counts_classes_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ preds,
                                                                 unsigned long long* __restrict__ counts, int64_t pixels, int M,
                                                                 AsrClassSet set, int include_bg) {
    __shared__ unsigned int part[4][ASR_MAX_CLASS_SET * kMaxIouMasks * 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slots = set.n * M * 4;
    for (int s = lane; s < slots; s += 64) part[wave][s] = 0u;
    __syncthreads();
    unsigned int* acc = part[wave];
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < pixels; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < pixels;
        const int t0 = in ? truth[i] : 0;
        for (int k = 0; k < set.n; ++k) {
            const int id = set.id[k];
            int tv = t0;
            if (include_bg && tv != id) tv = 0;  // utils.py:188-190
            const bool tc = in && tv == id, tb = in && tv == 0;
            for (int m = 0; m < M; ++m) {
                const int pv = in ? preds[((int64_t)k * M + m) * pixels + i] : 0;
                const bool pc = in && pv == id, pb = in && pv == 0;
                const unsigned int ic = __popcll(__ballot(tc && pc)), uc = __popcll(__ballot(tc || pc));
                const unsigned int ib = __popcll(__ballot(tb && pb)), ub = __popcll(__ballot(tb || pb));
                if (lane == 0) {
                    unsigned int* a = acc + (k * M + m) * 4;
                    a[0] += ic; a[1] += uc; a[2] += ib; a[3] += ub;
                }
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < slots; s += 256) {
        const unsigned long long v = (unsigned long long)part[0][s] + part[1][s] + part[2][s] + part[3][s];
        if (v) atomicAdd(counts + s, v);
    }
}

// One histogram add per lane (key -1: none).  Most pixels of a wave share one bin (the background): the lanes that hold lane
// 0's key add once, by popcount, the others one by one.  Every lane of the wave must reach the call.
__device__ __forceinline__ void label_hist_add(unsigned int* __restrict__ h, int key, int lane) {
    const int lead = __shfl(key, 0, 64);
    const unsigned long long same = __ballot(key == lead);
    if (key == lead) {
        if (key >= 0 && lane == __ffsll((long long)same) - 1) atomicAdd(h + key, (unsigned int)__popcll(same));
    } else if (key >= 0) {
        atomicAdd(h + key, 1u);
    }
}

// ---- threshold sweep: IoU counts of K threshold factors in one pass (threshold_tests.py:113-121) ------------------
// counts[s][k] equals asr_threshold_f32(image_s, NULL, factors[k]) followed by asr_iou_counts_i32: the pixel is predicted
// class_id when v > max_s * factors[k] (f32 product, strict >), else 0.  Each workgroup ranks the K thresholds in LDS
// (ties broken by factor index, so the ranks are a permutation of 0..K-1) and for each pixel finds r = #{thresholds < v}
// by binary search: the pixel is "on" for factor k exactly when rank[k] < r.  It bumps a histogram over (truth category,
// r), the category being the bits truth == class_id and truth == 0 after the include_bg remap; the finalize kernel turns
// the histograms into counts through per-rank prefix sums.  A negative maximum reverses the threshold order against the
// factor order; ranking the thresholds themselves covers that.  NaN inputs keep every index in range but are not exact.
constexpr int kSweepMaxFactors = 256;
constexpr int kSweepCats = 4;

// th[k] = mx * factors[k], sorted[rank[k]] = th[k]; every thread of the block takes part
__device__ __forceinline__ void sweep_rank(const float* __restrict__ factors, float mx, int K, float* __restrict__ th,
                                           int* __restrict__ rank, float* __restrict__ sorted) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) th[k] = mx * factors[k];
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float t = th[k];
        int r = 0;
        for (int j = 0; j < K; ++j) r += (th[j] < t) || (th[j] == t && j < k);
        r = r < K ? r : K - 1;                         // only NaN thresholds could break the permutation; keep it in range
        rank[k] = r;
        sorted[r] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void threshold_sweep_hist_kernel(const float* __restrict__ img, const int32_t* __restrict__ truth,
                                                                   const float* __restrict__ factors,
                                                                   const float* __restrict__ seg_minmax,
                                                                   unsigned long long* __restrict__ hist, int64_t per_seg,
                                                                   int64_t truth_stride, int K, int class_id, int include_bg) {
    __shared__ float th[kSweepMaxFactors], sorted[kSweepMaxFactors];
    __shared__ int rank[kSweepMaxFactors];
    __shared__ unsigned int sub[4][kSweepCats * (kSweepMaxFactors + 1)];     // one sub-histogram per wave
    const int seg = blockIdx.y;
    const int bins = kSweepCats * (K + 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 4 * kSweepCats * (kSweepMaxFactors + 1); i += 256) (&sub[0][0])[i] = 0u;
    sweep_rank(factors, seg_minmax[seg * 2 + 1], K, th, rank, sorted);
    const float* p = img + (int64_t)seg * per_seg;
    const int32_t* t = truth + (int64_t)seg * truth_stride;              // truth_stride 0: one label map for every image
    unsigned int* h = sub[wave];
    // the trip count is uniform over the workgroup, so every lane of a wave reaches label_hist_add together
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < per_seg; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        int key = -1;
        if (i < per_seg) {
            const float v = p[i];
            int lo = 0, hi = K;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sorted[mid] < v) lo = mid + 1; else hi = mid;
            }
            int tv = t[i];
            if (include_bg && tv != class_id) tv = 0;  // utils.py:188-190
            const int cat = (tv == class_id ? 1 : 0) | (tv == 0 ? 2 : 0);
            key = cat * (K + 1) + lo;
        }
        label_hist_add(h, key, lane);
    }
    __syncthreads();
    unsigned long long* g = hist + (int64_t)seg * bins;
    for (int b = threadIdx.x; b < bins; b += 256) {
        const unsigned long long v = (unsigned long long)sub[0][b] + sub[1][b] + sub[2][b] + sub[3][b];
        if (v) atomicAdd(g + b, v);
    }
}

// one workgroup per image, one thread per factor: the pixels of category c that are "off" for factor k are those with
// r <= rank[k] (a prefix of the histogram), the others are "on"
__global__ __launch_bounds__(256) void threshold_sweep_finalize_kernel(const float* __restrict__ factors,
                                                                       const float* __restrict__ seg_minmax,
                                                                       const unsigned long long* __restrict__ hist,
                                                                       long long* __restrict__ counts, int K, int class_id) {
    __shared__ float th[kSweepMaxFactors], sorted[kSweepMaxFactors];
    __shared__ int rank[kSweepMaxFactors];
    __shared__ unsigned long long pre[kSweepCats * (kSweepMaxFactors + 1)];
    const int seg = blockIdx.x;
    const int bins = kSweepCats * (K + 1);
    const unsigned long long* hs = hist + (int64_t)seg * bins;
    for (int b = threadIdx.x; b < bins; b += 256) pre[b] = hs[b];
    sweep_rank(factors, seg_minmax[seg * 2 + 1], K, th, rank, sorted);     // (its barriers also publish pre[])
    if (threadIdx.x < kSweepCats) {                                        // inclusive prefix sums, one category per thread
        unsigned long long run = 0;
        for (int r = 0; r <= K; ++r) {
            run += pre[threadIdx.x * (K + 1) + r];
            pre[threadIdx.x * (K + 1) + r] = run;
        }
    }
    __syncthreads();
    // what the thresholded mask holds: class_id when on, 0 when off (class_id == 0: always 0)
    const bool on_c = true, on_b = class_id == 0, off_c = class_id == 0, off_b = true;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int q = rank[k];
        unsigned long long ic = 0, uc = 0, ib = 0, ub = 0;
        for (int cat = 0; cat < kSweepCats; ++cat) {
            const unsigned long long off = pre[cat * (K + 1) + q];
            const unsigned long long on = pre[cat * (K + 1) + K] - off;
            const bool tc = cat & 1, tb = (cat >> 1) & 1;
            ic += (tc && on_c ? on : 0) + (tc && off_c ? off : 0);
            uc += (tc || on_c ? on : 0) + (tc || off_c ? off : 0);
            ib += (tb && on_b ? on : 0) + (tb && off_b ? off : 0);
            ub += (tb || on_b ? on : 0) + (tb || off_b ? off : 0);
        }
        long long* o = counts + ((int64_t)seg * K + k) * 4;
        o[0] = (long long)ic; o[1] = (long long)uc; o[2] = (long long)ib; o[3] = (long long)ub;
    }
}

// ---- per-label counts for Mean_IOU (utils.py:151-177) -----------------------------------------------------------
// counts[seg][0][l] = |truth == l|, [1][l] = |pred == l|, [2][l] = |truth == l & pred == l| for labels 0..255
// (union = [0] + [1] - [2]); labels outside 0..255 are not counted.
__global__ __launch_bounds__(256) void class_counts_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ pred,
                                                           unsigned long long* __restrict__ counts, int64_t per_seg) {
    __shared__ unsigned int hist[3 * 256];
    const int seg = blockIdx.y;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) hist[i] = 0;
    __syncthreads();
    const int32_t* t = truth + (int64_t)seg * per_seg;
    const int32_t* q = pred + (int64_t)seg * per_seg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_seg; i += (int64_t)gridDim.x * 256) {
        const int tv = t[i], pv = q[i];
        if (tv >= 0 && tv < 256) atomicAdd(hist + tv, 1u);
        if (pv >= 0 && pv < 256) atomicAdd(hist + 256 + pv, 1u);
        if (tv == pv && tv >= 0 && tv < 256) atomicAdd(hist + 512 + tv, 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += 256)
        if (hist[i]) atomicAdd(counts + (int64_t)seg * 768 + i, (unsigned long long)hist[i]);
}

// ---- label fusion: K per-class SR outputs of one image -> one label map (asr_fuse_labels_f32) ----------------------------
// Class k passes at a pixel exactly when its single-class mask is set there -- threshold_segment's own comparisons: s > max_k *
// th_factor (the f32 product, kept in LDS per class), or s >= m against its max map -- and the passing class with the greatest
// rank value (s, or the one f32 subtraction s - m) labels the pixel; the strict > below leaves equal values (-0.0 == +0.0 among
// them) to the lowest k, and 0 stays where no class passes.  Every plane is read once, four classes' loads in flight per
// thread.  With a ground truth the same pass counts what class_counts_kernel counts on the label it has just written: a
// wave's lanes that share lane 0's label (the background, mostly) add once by popcount, the others one by one, into a
// workgroup histogram in LDS that leaves through one 64-bit atomic per non-empty bin.  Out-of-range lanes carry key -1; the trip
// count is uniform over the workgroup, so every lane reaches the shuffles together.
template <bool HAS_MAX, bool HAS_TRUTH>
__global__ __launch_bounds__(256) void fuse_labels_kernel(const float* __restrict__ scores, const float* __restrict__ maxs,
                                                          const float* __restrict__ seg_minmax, const int32_t* __restrict__ truth,
                                                          int32_t* __restrict__ labels, unsigned long long* __restrict__ counts,
                                                          int64_t pixels, float th_factor, AsrClassSet set) {
    __shared__ float th[ASR_MAX_CLASS_SET];
    __shared__ unsigned int hist[HAS_TRUTH ? 3 * 256 : 1];
    const int K = set.n;
    if (!HAS_MAX && (int)threadIdx.x < K) th[threadIdx.x] = seg_minmax[threadIdx.x * 2 + 1] * th_factor;
    if (HAS_TRUTH)
        for (int i = threadIdx.x; i < 3 * 256; i += 256) hist[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < pixels; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < pixels;
        int lab = 0;
        if (in) {
            float best = 0.0f;
            bool have = false;
            for (int k0 = 0; k0 < K; k0 += 4) {
                float s[4], m[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool live = k0 + j < K;
                    s[j] = live ? scores[(int64_t)(k0 + j) * pixels + i] : 0.0f;
                    m[j] = (HAS_MAX && live) ? maxs[(int64_t)(k0 + j) * pixels + i] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k0 + j < K) {
                        const bool pass = HAS_MAX ? (s[j] >= m[j]) : (s[j] > th[k0 + j]);
                        const float r = HAS_MAX ? s[j] - m[j] : s[j];
                        if (pass && (!have || r > best)) { best = r; have = true; lab = set.id[k0 + j]; }
                    }
                }
            }
            labels[i] = lab;
        }
        if (HAS_TRUTH) {
            const int tv = in ? truth[i] : -1;
            const bool t_ok = in && tv >= 0 && tv < 256, p_ok = in && lab < 256;          // (lab >= 0 always)
            label_hist_add(hist, t_ok ? tv : -1, lane);
            label_hist_add(hist + 256, p_ok ? lab : -1, lane);
            label_hist_add(hist + 512, (t_ok && tv == lab) ? tv : -1, lane);
        }
    }
    if (HAS_TRUTH) {
        __syncthreads();
        for (int b = threadIdx.x; b < 3 * 256; b += 256)
            if (hist[b]) atomicAdd(counts + b, (unsigned long long)hist[b]);
    }
}

// ---- multi-label coupling (include/asr_hip.h, "multi-label coupling": the projection rule, statement for statement) -------------
// One thread per pixel of a group of G planes; plane j of the group is read and written at the same p by neighbouring lanes,
// so every access is coalesced.  The pixel's G positive parts sit in an LDS column [G][256] (lane stride 1: no bank conflict),
// touched by its own thread alone: no barrier.  Only a pixel with s > 1 sorts its column (insertion sort, at most G*(G-1)/2
// moves) and reads its values once more for the result; the others write what the column holds.  Every loop is counted.
// xb != NULL (the solve): the result also goes into the interior of the bordered copy the next forward launch reads -- pixel
// (Y, X) of plane b at xb[b * xb_plane + Y * xb_row + xb_first + X].  The unit is built without packed f32 and without contraction.
// stopped != NULL (the monitored solve): a stopped group -- the flag of its first member, they stop together -- is skipped.
// A kernel of the SR solver outside the solver's unit: csrc/isa_guard.py lets any kernel named sr_* hold packed-f32 instructions
// (sr.hip goes through the post-pass); this one must hold none, and what forbids them is THIS unit's flags (build.py: NO_PK_F32),
// not the name.  Moved into a packed-f32 unit it would need __attribute__((target("no-packed-fp32-ops"))) as sr.hip's
// SR_NO_PK_F32 kernels have.
__global__ __launch_bounds__(256) void sr_simplex_project_kernel(float* __restrict__ x, float* __restrict__ xb, int groups, int G,
                                                                 int64_t pixels, int W, int64_t xb_row, int64_t xb_first,
                                                                 int64_t xb_plane, const int* __restrict__ stopped) {
    extern __shared__ float sr_simplex_col[];
    float* const col = sr_simplex_col + threadIdx.x;
    for (int g = blockIdx.y; g < groups; g += gridDim.y) {
        if (stopped && stopped[g * G]) continue;
        float* const base = x + (int64_t)g * G * pixels;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
            float s = 0.0f;                            // 0 + a_0 is a_0
            for (int j = 0; j < G; ++j) {
                const float v = base[(int64_t)j * pixels + p];
                const float a = (v > 0.0f) ? v : 0.0f;
                col[j * 256] = a;
                s = s + a;
            }
            const bool over = s > 1.0f;
            float theta = 0.0f;
            if (over) {
                for (int i = 1; i < G; ++i) {          // descending
                    const float key = col[i * 256];
                    int k = i;
                    for (; k > 0; --k) {
                        const float prev = col[(k - 1) * 256];
                        if (!(prev < key)) break;
                        col[k * 256] = prev;
                    }
                    col[k * 256] = key;
                }
                float c = 0.0f;
                for (int k = 1; k <= G; ++k) {
                    const float u = col[(k - 1) * 256];
                    c = c + u;
                    const float t = (c - 1.0f) / (float)k;
                    if (u > t) theta = t;
                }
            }
            size_t ob = 0;
            if (xb) {
                const int64_t Y = p / W;
                ob = (size_t)((int64_t)g * G * xb_plane + Y * xb_row + xb_first + (p - Y * W));
            }
            for (int j = 0; j < G; ++j) {
                float r;
                if (over) {
                    const float v = base[(int64_t)j * pixels + p];
                    const float a = (v > 0.0f) ? v : 0.0f;
                    r = (a > theta) ? a - theta : 0.0f;
                } else {
                    r = col[j * 256];
                }
                base[(int64_t)j * pixels + p] = r;
                if (xb) xb[ob + (size_t)j * (size_t)xb_plane] = r;
            }
        }
    }
}

// ---- label fusion of a coupled solve (asr_fuse_labels_simplex_f32; include/asr_hip.h: the rule) -----------------------------
// The planes are shares of the pixel: s = ((S_0 + S_1) + ...) in index order, bg = 1 - s, the first k of greatest S_k wins when
// its share exceeds the background's.  One thread per pixel, every plane read once, four classes' loads in flight.
__global__ __launch_bounds__(256) void fuse_labels_simplex_kernel(const float* __restrict__ scores, int32_t* __restrict__ labels,
                                                                  int64_t pixels, AsrClassSet set) {
    const int K = set.n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
        float sum = 0.0f, best = 0.0f;
        int lab = 0;
        for (int k0 = 0; k0 < K; k0 += 4) {
            float s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = (k0 + j < K) ? scores[(int64_t)(k0 + j) * pixels + i] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < K) {
                    sum = (k0 + j == 0) ? s[j] : sum + s[j];
                    if (k0 + j == 0 || s[j] > best) { best = s[j]; lab = set.id[k0 + j]; }
                }
            }
        }
        const float bg = 1.0f - sum;
        labels[i] = (best > bg) ? lab : 0;
    }
}

// ---- label fusion swept over T threshold factors: counts only (asr_fuse_labels_sweep_counts_f32) --------------------------
// counts[j] is what fuse_labels_kernel<false, true> leaves at th_factor = factors[j]: the same f32 product max_k * factors[j],
// the same strict comparisons in the same order of k.  A predicted label is 0 or one of the K ids, so a workgroup counts in SLOTS
// (slot 0: label 0, slot k + 1: ids[k]) -- per factor a row of predicted and a row of agreeing pixels, K + 1 slots each, plus
// one 256-bin truth histogram that every factor shares -- and the finalize kernel scatters the slots into [T, 3, 256].  A thread
// keeps its pixel's K scores in its own column of an LDS tile (written and read by that thread alone: no barrier), loaded four
// planes at a time, and walks the factors over it; the thresholds th[j][k] sit in LDS and are read as broadcasts.  lo[k] is
// class k's lowest threshold over the factors: a wave none of whose pixels exceeds any lo[k] holds label 0 under every factor
// and adds its T rows by popcount, one lane per factor.  Dynamic LDS: tile [K][256] f32, th [T][K] f32, lo [K] f32,
// id [K + 1] i32, hist [T][2][K + 1] + [256] u32.  The trip count and T are uniform over the workgroup, so every lane reaches
// the ballots and label_hist_add together.
constexpr int kLabelSweepMaxFactors = 64;

__host__ __device__ constexpr size_t label_sweep_slots(int K, int T) { return (size_t)T * 2 * (size_t)(K + 1) + 256; }

__global__ __launch_bounds__(256) void fuse_labels_sweep_kernel(const float* __restrict__ scores, const float* __restrict__ seg_minmax,
                                                                const float* __restrict__ factors,
                                                                const int32_t* __restrict__ truth,
                                                                unsigned long long* __restrict__ slots, int64_t pixels, int T,
                                                                AsrClassSet set) {
    extern __shared__ unsigned int sweep_lds[];
    const int K = set.n, row = K + 1;
    float* tile = reinterpret_cast<float*>(sweep_lds);          // [K][256]
    float* th = tile + K * 256;                                 // [T][K]
    float* lo = th + T * K;                                     // [K]
    int* id = reinterpret_cast<int*>(lo + K);                   // [K + 1]
    unsigned int* hist = reinterpret_cast<unsigned int*>(id + row);     // [T][2][K + 1], then the truth's [256]
    unsigned int* thist = hist + T * 2 * row;
    const int nslots = (int)label_sweep_slots(K, T);
    for (int i = threadIdx.x; i < T * K; i += 256) th[i] = seg_minmax[(i % K) * 2 + 1] * factors[i / K];
    for (int i = threadIdx.x; i < nslots; i += 256) hist[i] = 0u;
    if ((int)threadIdx.x < row) {
        int v = 0;
        for (int k = 0; k < K; ++k) v = ((int)threadIdx.x == k + 1) ? set.id[k] : v;          // (no dynamic indexing of the argument)
        id[threadIdx.x] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        float m = th[threadIdx.x];
        for (int j = 1; j < T; ++j) m = fminf(m, th[j * K + threadIdx.x]);
        lo[threadIdx.x] = m;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    float* mine = tile + threadIdx.x;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < pixels; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < pixels;
        bool any = false;
        for (int k0 = 0; k0 < K; k0 += 4) {
            float s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = (in && k0 + j < K) ? scores[(int64_t)(k0 + j) * pixels + i] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < K) {
                    mine[(k0 + j) * 256] = s[j];
                    any = any || (in && s[j] > lo[k0 + j]);
                }
            }
        }
        const int tv = in ? truth[i] : -1;
        const bool t_ok = in && tv >= 0 && tv < 256;
        label_hist_add(thist, t_ok ? tv : -1, lane);
        if (__ballot(any) == 0ull) {                            // label 0 everywhere in the wave, whatever the factor
            const unsigned int n_in = (unsigned int)__popcll(__ballot(in)), n_zero = (unsigned int)__popcll(__ballot(in && tv == 0));
            if (lane < T) {
                if (n_in) atomicAdd(hist + lane * 2 * row, n_in);
                if (n_zero) atomicAdd(hist + lane * 2 * row + row, n_zero);
            }
            continue;
        }
        int t_slot = -1;                                        // the slot whose label the truth holds, if any
        if (t_ok)
            for (int q = 0; q < row; ++q) t_slot = (id[q] == tv) ? q : t_slot;
        for (int j = 0; j < T; ++j) {
            const float* tj = th + j * K;
            float best = 0.0f;
            int slot = 0;
            for (int k = 0; k < K; ++k) {
                const float s = mine[k * 256];
                if (s > tj[k] && (slot == 0 || s > best)) { best = s; slot = k + 1; }
            }
            const bool p_ok = in && id[slot] < 256;
            unsigned int* h = hist + j * 2 * row;
            label_hist_add(h, p_ok ? slot : -1, lane);
            label_hist_add(h + row, (p_ok && slot == t_slot) ? slot : -1, lane);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nslots; b += 256)
        if (hist[b]) atomicAdd(slots + b, (unsigned long long)hist[b]);
}

// one workgroup per factor, one thread per label: row 0 is the truth histogram, rows 1 and 2 take the slot of their label
__global__ __launch_bounds__(256) void fuse_labels_sweep_finalize_kernel(const unsigned long long* __restrict__ slots,
                                                                         long long* __restrict__ counts, int T, AsrClassSet set) {
    const int K = set.n, row = K + 1, j = blockIdx.x, l = threadIdx.x;
    int slot = l == 0 ? 0 : -1;
    for (int k = 0; k < K; ++k) slot = (set.id[k] == l) ? k + 1 : slot;
    const unsigned long long* h = slots + (size_t)j * 2 * row;
    long long* c = counts + (size_t)j * 768;
    c[l] = (long long)slots[(size_t)T * 2 * row + l];
    c[256 + l] = slot >= 0 ? (long long)h[slot] : 0;
    c[512 + l] = slot >= 0 ? (long long)h[row + slot] : 0;
}

// ---- trimap: squared distance to the nearest ground-truth label boundary (asr_boundary_dist2_u16) --------------------------
// A workgroup owns a 64-column x kDistRows-row output tile.  The strip it needs is the tile's rows +- r_max and the three
// 64-column words x0 - 64 .. x0 + 127 (r_max <= 64).  Phase 1: a wave walks down a word column of the strip holding the pixel
// above / at / below in registers, and one ballot per row packs the boundary predicate of its 64 pixels into a 64-bit word in
// LDS (pixels outside the image give 0 and are never a "different" neighbour).  Phase 2: every strip row gets, for each of the
// tile's 64 columns, the horizontal distance to the nearest set bit (two 64-bit windows ending / starting at the column, clz
// and ctz; 0..64, 255 = none) as one byte in LDS.  Phase 3: d2 = min over dy of dx(y + dy)^2 + dy^2, walking dy outwards
// from 0 and stopping once dy^2 alone is no better than the running minimum (which starts at r_max^2 + 1).  Integer throughout.
constexpr int kDistRows = 32;
constexpr int kDistMaxR = 64;
constexpr int kDistStrip = kDistRows + 2 * kDistMaxR;

__global__ __launch_bounds__(256) void boundary_dist2_kernel(const int32_t* __restrict__ truth, uint16_t* __restrict__ dist2,
                                                             int h, int w, int r) {
    __shared__ unsigned long long bits[kDistStrip * 3];
    __shared__ unsigned char dxs[kDistStrip * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * kDistRows;
    const int32_t* t = truth + (int64_t)blockIdx.z * h * w;
    uint16_t* o = dist2 + (int64_t)blockIdx.z * h * w;
    const int strip = kDistRows + 2 * r;                        // strip row s is image row y0 - r + s
    // phase 1: wave `wave` takes the strip rows [s_lo, s_hi) of each word column
    const int per_wave = (strip + 3) >> 2;
    const int s_lo = wave * per_wave, s_hi = min(strip, s_lo + per_wave);
    for (int k = 0; k < 3; ++k) {
        const int c = x0 - 64 + 64 * k + lane;
        const bool col_in = c >= 0 && c < w;
        auto at = [&](int y, int cc) { return (y >= 0 && y < h && cc >= 0 && cc < w) ? t[(int64_t)y * w + cc] : 0; };
        int y = y0 - r + s_lo;
        int up = at(y - 1, c), cur = at(y, c);
        for (int s = s_lo; s < s_hi; ++s, ++y) {                // (s_lo, s_hi are wave-uniform: every lane reaches the ballot)
            const int down = at(y + 1, c);
            const bool in = col_in && y >= 0 && y < h;
            const bool edge = in && ((y > 0 && up != cur) || (y + 1 < h && down != cur) || (c > 0 && at(y, c - 1) != cur) ||
                                     (c + 1 < w && at(y, c + 1) != cur));
            const unsigned long long word = __ballot(edge);
            if (lane == 0) bits[s * 3 + k] = word;
            up = cur;
            cur = down;
        }
    }
    __syncthreads();
    // phase 2: column j of the tile sits at bit j of the middle word; L holds the 64 bits ending at it, R the 64 starting at it
    for (int i = threadIdx.x; i < strip * 64; i += 256) {
        const int s = i >> 6, j = i & 63;
        const unsigned long long w0 = bits[s * 3], w1 = bits[s * 3 + 1], w2 = bits[s * 3 + 2];
        const unsigned long long L = (w1 << (63 - j)) | ((w0 >> j) >> 1);
        const unsigned long long R = (w1 >> j) | ((w2 << (63 - j)) << 1);
        int dl = 255, dr = 255;
        if (L) dl = __clzll((long long)L); else if ((w0 >> j) & 1ull) dl = 64;
        if (R) dr = __ffsll((long long)R) - 1; else if ((w2 >> j) & 1ull) dr = 64;
        dxs[i] = (unsigned char)min(dl, dr);
    }
    __syncthreads();
    // phase 3
    const int r2 = r * r;
    for (int row = wave; row < kDistRows; row += 4) {
        const int y = y0 + row, x = x0 + lane;
        if (y >= h) break;
        int best = r2 + 1;
        const int sc = row + r;
        for (int dy = 0; dy <= r && dy * dy < best; ++dy) {
            const int a = dxs[(sc - dy) * 64 + lane], b = dxs[(sc + dy) * 64 + lane];
            const int m = min(a, b);
            if (m != 255) best = min(best, m * m + dy * dy);
        }
        if (x < w) o[(int64_t)y * w + x] = (uint16_t)(best <= r2 ? best : 0xFFFF);
    }
}

// ---- trimap: per-label counts inside nested boundary bands (asr_band_class_counts_i32) -----------------------------------
// The distinct requested widths, ascending, are u_0 < ... < u_{U-1}.  A pixel's rank is the first i with d2 <= u_i^2 (none: the
// pixel is in no band); it is added once, as class_counts_kernel would add it, into row `rank` of a [U][3][256] workgroup
// histogram (label_hist_add: the lanes that share lane 0's bin add once).  Grid row p scores prediction p.  The rank
// histograms are summed into the first U of the B width slots of counts[p]; the finalize kernel then turns each bin's U rank
// values into prefix sums and writes the B cumulative counts in the caller's width order, in place (a thread owns one bin of
// one prediction in every slot, and reads all of it before it writes).
constexpr int kBandMaxWidths = 16;
constexpr int kBandMaxPreds = 8;

struct AsrBandSet {
    int n;                              // B: widths as the caller gave them
    int u;                              // U: distinct widths
    int w2[kBandMaxWidths];             // u_i^2, ascending
    int slot[kBandMaxWidths];           // widths[b] == u_{slot[b]}
};

__global__ __launch_bounds__(256) void band_hist_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ preds,
                                                        const uint16_t* __restrict__ dist2,
                                                        unsigned long long* __restrict__ counts, int64_t pixels,
                                                        int ignore_label, AsrBandSet set) {
    extern __shared__ unsigned int band_hist[];                 // [U][3][256]
    const int bins = set.u * 768;
    for (int i = threadIdx.x; i < bins; i += 256) band_hist[i] = 0u;
    __syncthreads();
    const int32_t* q = preds + (int64_t)blockIdx.y * pixels;
    const int lane = threadIdx.x & 63;
    // the trip count is uniform over the workgroup, so every lane of a wave reaches the ballots together
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < pixels; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        int rank = -1, tv = -1;
        if (i < pixels) {
            const int d2 = dist2[i];
            tv = truth[i];
            if (tv != ignore_label)
                for (int k = set.u - 1; k >= 0; --k) rank = d2 <= set.w2[k] ? k : rank;
        }
        if (__ballot(rank >= 0) == 0ull) continue;             // wave-uniform: most waves lie outside every band
        const int pv = rank >= 0 ? q[i] : -1;
        const bool t_ok = rank >= 0 && tv >= 0 && tv < 256, p_ok = rank >= 0 && pv >= 0 && pv < 256;
        const int base = (rank >= 0 ? rank : 0) * 768;         // label_hist_add compares keys: the rank goes into the key
        label_hist_add(band_hist, t_ok ? base + tv : -1, lane);
        label_hist_add(band_hist, p_ok ? base + 256 + pv : -1, lane);
        label_hist_add(band_hist, (t_ok && tv == pv) ? base + 512 + tv : -1, lane);
    }
    __syncthreads();
    unsigned long long* g = counts + (int64_t)blockIdx.y * set.n * 768;
    for (int b = threadIdx.x; b < bins; b += 256)
        if (band_hist[b]) atomicAdd(g + b, (unsigned long long)band_hist[b]);
}

__global__ __launch_bounds__(256) void band_finalize_kernel(long long* __restrict__ counts, int num_preds, AsrBandSet set) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_preds * 768) return;
    long long* c = counts + (int64_t)(i / 768) * set.n * 768 + (i % 768);
    long long pre[kBandMaxWidths];
    long long run = 0;
#pragma unroll
    for (int k = 0; k < kBandMaxWidths; ++k) {
        if (k < set.u) run += c[(int64_t)k * 768];
        pre[k] = run;
    }
    for (int b = 0; b < set.n; ++b) {
        long long v = 0;
#pragma unroll
        for (int k = 0; k < kBandMaxWidths; ++k) v = (set.slot[b] == k) ? pre[k] : v;     // (no dynamic register indexing)
        c[(int64_t)b * 768] = v;
    }
}

// ---- binned counts: class_counts over the pixels whose value u lies at or below each of B edges (asr_binned_class_counts_f32) --
// Bin j is {p : u[p] <= edges[j]} (one f32 compare: NaN on either side is in no bin), truth != ignore_label; the bins are
// independent of each other, so the edges need no order and a pixel is added once per bin that holds it, as
// class_counts_kernel would add it, into row j of a [B][3][256] workgroup histogram (label_hist_add).  The edges come from
// device memory (a selection that never left the device) and are staged in LDS once per workgroup.  Grid row p scores
// prediction p; the loop over the bins runs to num_bins for every lane, and a bin that holds no pixel of the wave is skipped
// wave-uniformly.
constexpr int kBinnedMaxBins = 16;
constexpr int kBinnedMaxPreds = 8;

__global__ __launch_bounds__(256) void binned_hist_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ preds,
                                                          const float* __restrict__ u, const float* __restrict__ edges,
                                                          unsigned long long* __restrict__ counts, int64_t pixels,
                                                          int ignore_label, int num_bins) {
    extern __shared__ unsigned int binned_hist[];               // [B][3][256]
    __shared__ float edge[kBinnedMaxBins];
    const int bins = num_bins * 768;
    for (int i = threadIdx.x; i < bins; i += 256) binned_hist[i] = 0u;
    if (threadIdx.x < num_bins) edge[threadIdx.x] = edges[threadIdx.x];
    __syncthreads();
    const int32_t* q = preds + (int64_t)blockIdx.y * pixels;
    const int lane = threadIdx.x & 63;
    // the trip count is uniform over the workgroup, so every lane of a wave reaches the ballots and label_hist_add together
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < pixels; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < pixels;
        const int tv = in ? truth[i] : -1, pv = in ? q[i] : -1;
        const float uv = in ? u[i] : 0.0f;
        const bool live = in && (ignore_label == -1 || tv != ignore_label);
        const bool t_ok = tv >= 0 && tv < 256, p_ok = pv >= 0 && pv < 256;
        for (int j = 0; j < num_bins; ++j) {
            const bool held = live && uv <= edge[j];
            if (__ballot(held) == 0ull) continue;              // wave-uniform
            const int base = j * 768;                           // label_hist_add compares keys: the bin goes into the key
            label_hist_add(binned_hist, (held && t_ok) ? base + tv : -1, lane);
            label_hist_add(binned_hist, (held && p_ok) ? base + 256 + pv : -1, lane);
            label_hist_add(binned_hist, (held && t_ok && tv == pv) ? base + 512 + tv : -1, lane);
        }
    }
    __syncthreads();
    unsigned long long* g = counts + (int64_t)blockIdx.y * bins;
    for (int b = threadIdx.x; b < bins; b += 256)
        if (binned_hist[b]) atomicAdd(g + b, (unsigned long long)binned_hist[b]);
}

// ---- confusion matrix: (truth label, predicted label) pair counts of label maps (asr_confusion_counts_i32) ----------------
// bin(v) = v for 0 <= v < L, else L ("other").  A pixel is one key bin(t) * (L + 1) + bin(p), added with label_hist_add into a
// workgroup histogram of (L + 1)^2 bins in LDS (most pixels of a wave are background on background: one popcount add); every
// non-empty bin then leaves through one 64-bit atomic.  Grid row p scores prediction p.  A thread takes kConfPerThread pixels
// per trip, a workgroup stride apart, and loads them all before the first add: at 512^2 a grid row's workgroup has 4096
// pixels, so the kernel is a few dependent load round trips long and its time goes with their number, not with LDS or HBM.
constexpr int kConfPerThread = ASR_CONFUSION_SPAN / 256;
static_assert(kConfPerThread * 256 == ASR_CONFUSION_SPAN, "a workgroup's trip is a whole number of pixels per thread");

__device__ __forceinline__ int conf_bin(int v, int L) { return (unsigned int)v < (unsigned int)L ? v : L; }

__global__ __launch_bounds__(256) void confusion_hist_kernel(const int32_t* __restrict__ truth, const int32_t* __restrict__ preds,
                                                             unsigned long long* __restrict__ counts, int64_t pixels, int L) {
    extern __shared__ unsigned int conf_hist[];                 // [L + 1][L + 1]
    const int side = L + 1, bins = side * side;
    for (int i = threadIdx.x; i < bins; i += 256) conf_hist[i] = 0u;
    __syncthreads();
    const int32_t* q = preds + (int64_t)blockIdx.y * pixels;
    const int lane = threadIdx.x & 63;
    // the trip count is uniform over the workgroup, so every lane of a wave reaches label_hist_add together
    for (int64_t i0 = (int64_t)blockIdx.x * ASR_CONFUSION_SPAN; i0 < pixels; i0 += (int64_t)gridDim.x * ASR_CONFUSION_SPAN) {
        int key[kConfPerThread];
#pragma unroll
        for (int j = 0; j < kConfPerThread; ++j) {
            const int64_t i = i0 + j * 256 + threadIdx.x;
            const bool in = i < pixels;
            const int tv = in ? truth[i] : 0, pv = in ? q[i] : 0;
            key[j] = in ? conf_bin(tv, L) * side + conf_bin(pv, L) : -1;
        }
#pragma unroll
        for (int j = 0; j < kConfPerThread; ++j) label_hist_add(conf_hist, key[j], lane);
    }
    __syncthreads();
    unsigned long long* g = counts + (int64_t)blockIdx.y * bins;
    for (int b = threadIdx.x; b < bins; b += 256)
        if (conf_hist[b]) atomicAdd(g + b, (unsigned long long)conf_hist[b]);
}

// ---- last_activation: softmax / sigmoid over the class axis (model.py:124-125) ----------------------
__device__ __forceinline__ void activate_row(const float* row, float* o, int classes, int kind) {     // o may be row
    if (kind == 1) {                       // softmax: exp(x - max) / sum
        float mx = row[0];
        for (int c = 1; c < classes; ++c) mx = fmaxf(mx, row[c]);
        float sum = 0.f;
        for (int c = 0; c < classes; ++c) sum += expf(row[c] - mx);
        for (int c = 0; c < classes; ++c) o[c] = expf(row[c] - mx) / sum;
    } else {                               // sigmoid
        for (int c = 0; c < classes; ++c) o[c] = 1.0f / (1.0f + expf(-row[c]));
    }
}

// Rows of `classes` floats (84 bytes for 21 classes) walked by one thread each are 64-way strided gathers and scatters
// (measured 0.44 TB/s on the [100,128,128,21] logits of BASELINE configs[2]); like argmax_kernel, a workgroup moves its
// 256 rows through LDS with coalesced loads and stores and the threads work on the LDS rows, in place (STAGED), or, beyond
// the LDS tile, each thread on its own row in global memory.
template <bool STAGED>
__global__ __launch_bounds__(256) void class_activation_kernel(const float* __restrict__ logits, float* __restrict__ out,
                                                              int64_t pixels, int classes, int kind) {
    __shared__ float tile[STAGED ? 256 * kMaxStageClasses : 1];
    for (int64_t first = (int64_t)blockIdx.x * 256; first < pixels; first += (int64_t)gridDim.x * 256) {
        const int64_t p = first + threadIdx.x;
        float* o = STAGED ? stage_rows(logits, first, pixels, classes, tile) : out + p * classes;
        // in place on an LDS row, every o[c] is written after the last read of row[c'] it needs: softmax re-reads row[c]
        // right before overwriting it
        if (p < pixels) activate_row(STAGED ? o : logits + p * classes, o, classes, kind);
        if (STAGED) {
            __syncthreads();
            const int64_t n = min((int64_t)256, pixels - first) * classes;
            float* dst = out + first * classes;
            for (int64_t i = threadIdx.x; i < n; i += 256) dst[i] = tile[i];
            __syncthreads();
        }
    }
}

// ---- confidence per pixel (asr_opm_confidence_f32; include/asr_hip.h: the rule) ------------------------------------------
// The statements of activate_row's softmax on the same operands -- the row maximum by fmaxf in class order, the sum of
// expf(z - max) in class order, one division per entry -- for the largest entry (expf(0) is 1) and the second largest.
__device__ __forceinline__ float confidence_row(const float* row, int classes, int kind) {
    float mx = row[0];
    for (int c = 1; c < classes; ++c) mx = fmaxf(mx, row[c]);
    float sum = 0.f;
    for (int c = 0; c < classes; ++c) sum += expf(row[c] - mx);
    const float top = 1.0f / sum;
    if (kind == ASR_CONF_MAXPROB) return top;
    float m1 = row[0], m2 = -__builtin_inff();          // the two largest logits, with multiplicity
    for (int c = 1; c < classes; ++c) {
        const float v = row[c];
        if (v > m1) { m2 = m1; m1 = v; }
        else if (v > m2) m2 = v;
    }
    return top - expf(m2 - mx) / sum;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void opm_confidence_kernel(const float* __restrict__ logits, float* __restrict__ out,
                                                            int64_t pixels, int classes, int kind) {
    __shared__ float tile[STAGED ? 256 * kMaxStageClasses : 1];
    for (int64_t first = (int64_t)blockIdx.x * 256; first < pixels; first += (int64_t)gridDim.x * 256) {
        const int64_t p = first + threadIdx.x;
        const float* row = STAGED ? stage_rows(logits, first, pixels, classes, tile) : logits + p * classes;
        if (p < pixels) out[p] = confidence_row(row, classes, kind);
        if (STAGED) __syncthreads();
    }
}

int stream_grid(int64_t n) {
    int64_t g = asr_cdiv(n, 256);
    return (int)(g < 2048 ? (g > 0 ? g : 1) : 2048);
}

}  // namespace

extern "C" int asr_minmax_f32(const float* x, float* out_minmax, int64_t per_segment, int segments, asr_stream_t stream) {
    ASR_REQUIRE(x && out_minmax, "asr_minmax_f32: null pointer");
    ASR_REQUIRE(per_segment > 0 && segments > 0, "asr_minmax_f32: empty input (per_segment=%lld segments=%d)",
                (long long)per_segment, segments);
    ASR_REQUIRE(segments <= 65535, "asr_minmax_f32: more than 65535 segments");
    hipLaunchKernelGGL(minmax_init_kernel, dim3((unsigned)asr_cdiv(segments, 256)), dim3(256), 0, asr_stream(stream), out_minmax, segments);
    ASR_LAUNCH_CHECK();
    // ~16 K elements per workgroup, at most ~1024 workgroups in the launch
    long long per_wg = asr_cdiv(per_segment, 16384);
    const long long cap = segments >= 1024 ? 1 : 1024 / segments;
    if (per_wg > cap) per_wg = cap;
    hipLaunchKernelGGL(minmax_kernel, dim3((unsigned)per_wg, (unsigned)segments), dim3(1024), 0, asr_stream(stream), x, out_minmax,
                       per_segment);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_argmax_i32(const float* logits, int32_t* out, int64_t pixels, int classes, asr_stream_t stream) {
    ASR_REQUIRE(logits && out, "asr_argmax_i32: null pointer");
    ASR_REQUIRE(pixels > 0 && classes > 0, "asr_argmax_i32: bad shape");
    if (classes <= kMaxStageClasses)
        hipLaunchKernelGGL(argmax_kernel<true>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out, pixels, classes);
    else
        hipLaunchKernelGGL(argmax_kernel<false>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out, pixels, classes);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// Every OPM entry point launches here, after its own argument checks: the single-class ones with a set of one, so that they
// and asr_opm_classes_f32 with K = 1 cannot run different kernels.  argmax / slice_max take all copies * pixels_per_copy pixels
// as one copy; slice computes the per-copy extrema first (once for all classes of the set).
static int opm_launch(int mode, const float* logits, const AsrClassSet& set, float* class_masks, float* max_masks, float* minmax_ws,
                      int copies, int64_t pixels_per_copy, int classes, int64_t class_stride, float new_min, float new_max,
                      asr_stream_t stream) {
    hipStream_t s = asr_stream(stream);
    const int64_t pixels = (int64_t)copies * pixels_per_copy;
    // A slice of one class reads one float per row: on logits [16, 128, 128, 21] staging whole rows through LDS takes 8.68 us, the
    // walk from global memory 4.20 us (measured, DESIGN.md "Class sets"), so a set of one takes <SLICE, false>.  Chosen here, so
    // that asr_opm_slice_f32 and a one-id asr_opm_classes_f32 launch the same instantiation.
    const bool staged = classes <= kMaxStageClasses && !(mode == ASR_OPM_SLICE && set.n == 1);
#define ASR_OPM_CLASSES_LAUNCH(M, grid, per, ws)                                                                              \
    do {                                                                                                                    \
        if (staged)                                                                                                         \
            hipLaunchKernelGGL((opm_classes_kernel<M, true>), grid, dim3(256), 0, s, logits, class_masks, max_masks, ws, per, \
                               classes, class_stride, set, new_min, new_max);                                               \
        else                                                                                                                \
            hipLaunchKernelGGL((opm_classes_kernel<M, false>), grid, dim3(256), 0, s, logits, class_masks, max_masks, ws,     \
                               per, classes, class_stride, set, new_min, new_max);                                          \
    } while (0)
    if (mode == ASR_OPM_ARGMAX) {
        ASR_OPM_CLASSES_LAUNCH(ASR_OPM_ARGMAX, dim3(stream_grid(pixels)), pixels, nullptr);
    } else if (mode == ASR_OPM_SLICE_MAX) {
        ASR_OPM_CLASSES_LAUNCH(ASR_OPM_SLICE_MAX, dim3(stream_grid(pixels)), pixels, nullptr);
    } else {
        const int rc = asr_minmax_f32(logits, minmax_ws, pixels_per_copy * classes, copies, stream);
        if (rc != ASR_OK) return rc;
        ASR_OPM_CLASSES_LAUNCH(ASR_OPM_SLICE, dim3(stream_grid(pixels_per_copy), copies), pixels_per_copy, minmax_ws);
    }
#undef ASR_OPM_CLASSES_LAUNCH
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_opm_argmax_f32(const float* logits, float* class_mask, int64_t pixels, int classes, int class_id,
                                  asr_stream_t stream) {
    ASR_REQUIRE(logits && class_mask, "asr_opm_argmax_f32: null pointer");
    ASR_REQUIRE(pixels > 0 && classes > 0 && class_id >= 0 && class_id < classes, "asr_opm_argmax_f32: bad shape/class");
    return opm_launch(ASR_OPM_ARGMAX, logits, asr_one_class(class_id), class_mask, nullptr, nullptr, 1, pixels, classes, pixels, 0.0f,
                      0.0f, stream);
}

extern "C" int asr_opm_slice_max_f32(const float* logits, float* class_mask, float* max_mask, int64_t pixels, int classes,
                                     int class_id, asr_stream_t stream) {
    ASR_REQUIRE(logits && class_mask && max_mask, "asr_opm_slice_max_f32: null pointer");
    ASR_REQUIRE(pixels > 0 && classes > 1 && class_id >= 0 && class_id < classes, "asr_opm_slice_max_f32: bad shape/class");
    return opm_launch(ASR_OPM_SLICE_MAX, logits, asr_one_class(class_id), class_mask, max_mask, nullptr, 1, pixels, classes, pixels,
                      0.0f, 0.0f, stream);
}

extern "C" int asr_opm_slice_f32(const float* logits, float* class_mask, float* minmax_ws, int copies,
                                 int64_t pixels_per_copy, int classes, int class_id, float new_min, float new_max,
                                 asr_stream_t stream) {
    ASR_REQUIRE(logits && class_mask && minmax_ws, "asr_opm_slice_f32: null pointer");
    ASR_REQUIRE(copies > 0 && copies <= 65535 && pixels_per_copy > 0 && classes > 0 && class_id >= 0 && class_id < classes,
                "asr_opm_slice_f32: bad shape/class");
    return opm_launch(ASR_OPM_SLICE, logits, asr_one_class(class_id), class_mask, nullptr, minmax_ws, copies, pixels_per_copy, classes,
                      (int64_t)copies * pixels_per_copy, new_min, new_max, stream);
}

extern "C" int asr_threshold_f32(const float* image, const float* th_mask, float* minmax_ws, int32_t* out,
                                 int64_t per_segment, int segments, float th_factor, int th_value,
                                 asr_stream_t stream) {
    ASR_REQUIRE(image && out, "asr_threshold_f32: null pointer");
    ASR_REQUIRE(per_segment > 0 && segments > 0 && segments <= 65535, "asr_threshold_f32: bad shape");
    if (!th_mask) {
        ASR_REQUIRE(minmax_ws, "asr_threshold_f32: minmax workspace required without th_mask");
        int rc = asr_minmax_f32(image, minmax_ws, per_segment, segments, stream);
        if (rc != ASR_OK) return rc;
    }
    hipLaunchKernelGGL(threshold_kernel, dim3(stream_grid(per_segment), segments), dim3(256), 0, asr_stream(stream),
                       image, th_mask, minmax_ws, out, per_segment, th_factor, th_value);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

static int iou_counts_common(const char* fn, const int32_t* truth, const int32_t* pred, int64_t* counts, int64_t per_segment,
                             int64_t truth_stride, int segments, int class_id, int include_bg, asr_stream_t stream) {
    ASR_REQUIRE(truth && pred && counts, "%s: null pointer", fn);
    ASR_REQUIRE(per_segment > 0 && segments > 0 && segments <= 65535, "%s: bad shape", fn);
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 4 * segments, s));
    hipLaunchKernelGGL(iou_counts_kernel, dim3(stream_grid(per_segment) > 64 ? 64 : stream_grid(per_segment), segments),
                       dim3(256), 0, s, truth, pred, reinterpret_cast<unsigned long long*>(counts), per_segment, truth_stride,
                       class_id, include_bg);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_iou_counts_i32(const int32_t* truth, const int32_t* pred, int64_t* counts, int64_t per_segment,
                                  int segments, int class_id, int include_bg, asr_stream_t stream) {
    return iou_counts_common("asr_iou_counts_i32", truth, pred, counts, per_segment, per_segment, segments, class_id, include_bg,
                             stream);
}

extern "C" int asr_iou_counts_shared_truth_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels,
                                               int num_preds, int class_id, int include_bg, asr_stream_t stream) {
    return iou_counts_common("asr_iou_counts_shared_truth_i32", truth, preds, counts, pixels, 0, num_preds, class_id,
                             include_bg, stream);
}

extern "C" int asr_opm_classes_f32(const float* logits, const int* ids, int K, int mode, float* class_masks, float* max_masks,
                                   float* minmax_ws, int copies, int64_t pixels_per_copy, int classes, int64_t class_stride,
                                   float new_min, float new_max, asr_stream_t stream) {
    AsrClassSet set;
    int rc = asr_class_set("asr_opm_classes_f32", ids, K, classes, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(logits && class_masks, "asr_opm_classes_f32: null pointer");
    ASR_REQUIRE(mode == ASR_OPM_ARGMAX || mode == ASR_OPM_SLICE || mode == ASR_OPM_SLICE_MAX,
                "asr_opm_classes_f32: mode %d (0 argmax, 1 slice, 2 slice_max)", mode);
    ASR_REQUIRE(copies > 0 && copies <= 65535 && pixels_per_copy > 0 && classes > 0, "asr_opm_classes_f32: bad shape");
    const int64_t pixels = (int64_t)copies * pixels_per_copy;
    ASR_REQUIRE(K == 1 || class_stride >= pixels, "asr_opm_classes_f32: class_stride %lld < %lld pixels (planes would overlap)",
                (long long)class_stride, (long long)pixels);
    ASR_REQUIRE(mode != ASR_OPM_SLICE_MAX || (max_masks && classes > 1),
                "asr_opm_classes_f32: slice_max needs max_masks and classes > 1");
    ASR_REQUIRE(mode != ASR_OPM_SLICE || minmax_ws, "asr_opm_classes_f32: slice needs minmax_ws");
    return opm_launch(mode, logits, set, class_masks, max_masks, minmax_ws, copies, pixels_per_copy, classes, class_stride, new_min,
                      new_max, stream);
}

extern "C" int asr_threshold_classes_f32(const float* image, const float* th_mask, float* minmax_ws, int32_t* out,
                                         int64_t per_segment, int K, float th_factor, const int* th_values,
                                         asr_stream_t stream) {
    AsrClassSet values;
    int rc = asr_class_set("asr_threshold_classes_f32", th_values, K, 0, &values);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(image && out, "asr_threshold_classes_f32: null pointer");
    ASR_REQUIRE(per_segment > 0, "asr_threshold_classes_f32: bad shape");
    if (!th_mask) {
        ASR_REQUIRE(minmax_ws, "asr_threshold_classes_f32: minmax workspace required without th_mask");
        rc = asr_minmax_f32(image, minmax_ws, per_segment, K, stream);
        if (rc != ASR_OK) return rc;
    }
    hipLaunchKernelGGL(threshold_classes_kernel, dim3(stream_grid(per_segment), K), dim3(256), 0, asr_stream(stream), image,
                       th_mask, minmax_ws, out, per_segment, th_factor, values);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_iou_counts_classes_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels, int K,
                                          int M, const int* ids, int include_bg, asr_stream_t stream) {
    AsrClassSet set;
    int rc = asr_class_set("asr_iou_counts_classes_i32", ids, K, 0, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(truth && preds && counts, "asr_iou_counts_classes_i32: null pointer");
    ASR_REQUIRE(pixels > 0 && M >= 1 && M <= kMaxIouMasks, "asr_iou_counts_classes_i32: bad shape (pixels=%lld, M=%d; 1..%d masks)",
                (long long)pixels, M, kMaxIouMasks);
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 4 * (size_t)K * (size_t)M, s));
    const int grid = stream_grid(pixels) > 128 ? 128 : stream_grid(pixels);
    hipLaunchKernelGGL(iou_counts_classes_kernel, dim3(grid), dim3(256), 0, s, truth, preds,
                       reinterpret_cast<unsigned long long*>(counts), pixels, M, set, include_bg);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_fuse_labels_f32(const float* scores, const float* max_scores, float* minmax_ws, const int32_t* truth,
                                   int32_t* labels, int64_t* counts, int64_t pixels, int K, float th_factor, const int* ids,
                                   int classes, asr_stream_t stream) {
    AsrClassSet set;
    int rc = asr_label_set("asr_fuse_labels_f32", ids, K, classes, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(scores && labels, "asr_fuse_labels_f32: null pointer");
    ASR_REQUIRE(pixels > 0, "asr_fuse_labels_f32: bad shape");
    ASR_REQUIRE(!truth == !counts, "asr_fuse_labels_f32: truth and counts go together (both or neither)");
    hipStream_t s = asr_stream(stream);
    if (!max_scores) {
        ASR_REQUIRE(minmax_ws, "asr_fuse_labels_f32: minmax workspace required without max_scores");
        rc = asr_minmax_f32(scores, minmax_ws, pixels, K, stream);
        if (rc != ASR_OK) return rc;
    }
    if (counts) ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 768, s));
    const int grid = stream_grid(pixels) > 1024 ? 1024 : stream_grid(pixels);
    auto* c = reinterpret_cast<unsigned long long*>(counts);
#define ASR_FUSE_LAUNCH(MX, TR) \
    hipLaunchKernelGGL((fuse_labels_kernel<MX, TR>), dim3(grid), dim3(256), 0, s, scores, max_scores, minmax_ws, truth, labels, c, \
                       pixels, th_factor, set)
    if (max_scores) {
        if (truth) ASR_FUSE_LAUNCH(true, true); else ASR_FUSE_LAUNCH(true, false);
    } else {
        if (truth) ASR_FUSE_LAUNCH(false, true); else ASR_FUSE_LAUNCH(false, false);
    }
#undef ASR_FUSE_LAUNCH
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

int asr_simplex_project_launch(hipStream_t s, float* x, float* xb, int groups, int G, int64_t pixels, int W, int64_t xb_row,
                               int64_t xb_first, int64_t xb_plane, const int* stopped) {
    const int64_t blocks = asr_cdiv(pixels, 256);
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(sr_simplex_project_kernel, grid, dim3(256), sizeof(float) * 256 * (size_t)G, s, x, xb, groups, G, pixels, W,
                       xb_row, xb_first, xb_plane, stopped);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_fuse_labels_simplex_f32(const float* scores, const int* ids, int K, int32_t* labels, int64_t pixels,
                                           asr_stream_t stream) {
    AsrClassSet set;
    const int rc = asr_label_set("asr_fuse_labels_simplex_f32", ids, K, 0, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(scores && labels, "asr_fuse_labels_simplex_f32: null pointer");
    ASR_REQUIRE(pixels > 0, "asr_fuse_labels_simplex_f32: bad shape");
    hipLaunchKernelGGL(fuse_labels_simplex_kernel, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), scores, labels, pixels,
                       set);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" size_t asr_fuse_labels_sweep_workspace_bytes(int K, int num_factors) {
    if (K <= 0 || num_factors <= 0) return 0;
    return sizeof(unsigned long long) * label_sweep_slots(K, num_factors) + sizeof(float) * 2 * (size_t)K;
}

extern "C" int asr_fuse_labels_sweep_counts_f32(const float* scores, const int32_t* truth, const float* factors, void* workspace,
                                                size_t workspace_bytes, int64_t* counts, int64_t pixels, int K, int num_factors,
                                                const int* ids, int classes, asr_stream_t stream) {
    AsrClassSet set;
    int rc = asr_label_set("asr_fuse_labels_sweep_counts_f32", ids, K, classes, &set);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(scores && truth && factors && workspace && counts, "asr_fuse_labels_sweep_counts_f32: null pointer");
    ASR_REQUIRE(pixels > 0, "asr_fuse_labels_sweep_counts_f32: bad shape");
    ASR_REQUIRE(num_factors >= 1 && num_factors <= kLabelSweepMaxFactors,
                "asr_fuse_labels_sweep_counts_f32: %d threshold factors (1..%d)", num_factors, kLabelSweepMaxFactors);
    ASR_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % sizeof(unsigned long long) == 0,
                "asr_fuse_labels_sweep_counts_f32: workspace not aligned to 8 bytes");
    const size_t need = asr_fuse_labels_sweep_workspace_bytes(K, num_factors);
    if (workspace_bytes < need) {
        asr_set_error("asr_fuse_labels_sweep_counts_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    hipStream_t s = asr_stream(stream);
    auto* slots = reinterpret_cast<unsigned long long*>(workspace);
    const size_t slot_bytes = sizeof(unsigned long long) * label_sweep_slots(K, num_factors);
    float* minmax = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + slot_bytes);
    rc = asr_minmax_f32(scores, minmax, pixels, K, stream);
    if (rc != ASR_OK) return rc;
    ASR_HIP_CHECK(hipMemsetAsync(slots, 0, slot_bytes, s));
    // every workgroup flushes its own slots: at most two workgroups per compute unit's worth of them
    const int grid = stream_grid(pixels) > 512 ? 512 : stream_grid(pixels);
    const size_t lds = sizeof(float) * ((size_t)K * 256 + (size_t)num_factors * K + K) + sizeof(int) * (size_t)(K + 1) +
                       sizeof(unsigned int) * label_sweep_slots(K, num_factors);
    hipLaunchKernelGGL(fuse_labels_sweep_kernel, dim3(grid), dim3(256), lds, s, scores, minmax, factors, truth, slots, pixels,
                       num_factors, set);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(fuse_labels_sweep_finalize_kernel, dim3(num_factors), dim3(256), 0, s, slots,
                       reinterpret_cast<long long*>(counts), num_factors, set);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" size_t asr_threshold_sweep_workspace_bytes(int segments, int num_factors) {
    if (segments <= 0 || num_factors <= 0) return 0;
    return sizeof(unsigned long long) * kSweepCats * (size_t)(num_factors + 1) * (size_t)segments +
           sizeof(float) * 2 * (size_t)segments;
}

extern "C" int asr_threshold_sweep_iou_counts_f32(const float* images, const int32_t* truth, const float* factors,
                                                  void* workspace, size_t workspace_bytes, int64_t* counts,
                                                  int64_t per_segment, int segments, int num_factors, int shared_truth,
                                                  int class_id, int include_bg, asr_stream_t stream) {
    ASR_REQUIRE(images && truth && factors && workspace && counts, "asr_threshold_sweep_iou_counts_f32: null pointer");
    ASR_REQUIRE(per_segment > 0 && segments > 0 && segments <= 65535,
                "asr_threshold_sweep_iou_counts_f32: bad shape (per_segment=%lld, segments=%d; at most 65535 segments)",
                (long long)per_segment, segments);
    ASR_REQUIRE(num_factors >= 1 && num_factors <= kSweepMaxFactors,
                "asr_threshold_sweep_iou_counts_f32: %d threshold factors (1..%d)", num_factors, kSweepMaxFactors);
    const size_t need = asr_threshold_sweep_workspace_bytes(segments, num_factors);
    if (workspace_bytes < need) {
        asr_set_error("asr_threshold_sweep_iou_counts_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return ASR_ERR_WORKSPACE;
    }
    hipStream_t s = asr_stream(stream);
    auto* hist = reinterpret_cast<unsigned long long*>(workspace);
    const size_t hist_bytes = sizeof(unsigned long long) * kSweepCats * (size_t)(num_factors + 1) * (size_t)segments;
    float* minmax = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + hist_bytes);
    int rc = asr_minmax_f32(images, minmax, per_segment, segments, stream);
    if (rc != ASR_OK) return rc;
    ASR_HIP_CHECK(hipMemsetAsync(hist, 0, hist_bytes, s));
    // 64..256 workgroups per image, fewer per image as the images get more: each one flushes its own histogram
    int per_image = 1024 / segments;
    per_image = per_image < 64 ? 64 : (per_image > 256 ? 256 : per_image);
    const int grid = stream_grid(per_segment) > per_image ? per_image : stream_grid(per_segment);
    hipLaunchKernelGGL(threshold_sweep_hist_kernel, dim3(grid, segments), dim3(256), 0, s, images, truth, factors, minmax, hist,
                       per_segment, shared_truth ? (int64_t)0 : per_segment, num_factors, class_id, include_bg);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(threshold_sweep_finalize_kernel, dim3(segments), dim3(256), 0, s, factors, minmax, hist,
                       reinterpret_cast<long long*>(counts), num_factors, class_id);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_minmax_normalize_f32(const float* x, float* out, float* minmax_ws, int64_t per_segment, int segments,
                                        float new_min, float new_max, asr_stream_t stream) {
    ASR_REQUIRE(x && out && minmax_ws, "asr_minmax_normalize_f32: null pointer");
    int rc = asr_minmax_f32(x, minmax_ws, per_segment, segments, stream);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(minmax_normalize_kernel, dim3(stream_grid(per_segment), segments), dim3(256), 0, asr_stream(stream), x, out,
                       minmax_ws, per_segment, new_min, new_max);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_class_counts_i32(const int32_t* truth, const int32_t* pred, int64_t* counts, int64_t per_segment,
                                    int segments, asr_stream_t stream) {
    ASR_REQUIRE(truth && pred && counts, "asr_class_counts_i32: null pointer");
    ASR_REQUIRE(per_segment > 0 && segments > 0 && segments <= 65535, "asr_class_counts_i32: bad shape");
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 768 * (size_t)segments, s));
    const int grid = stream_grid(per_segment) > 64 ? 64 : stream_grid(per_segment);
    hipLaunchKernelGGL(class_counts_kernel, dim3(grid, segments), dim3(256), 0, s, truth, pred,
                       reinterpret_cast<unsigned long long*>(counts), per_segment);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_class_activation_f32(const float* logits, float* out, int64_t pixels, int classes, int kind,
                                        asr_stream_t stream) {
    ASR_REQUIRE(logits && out, "asr_class_activation_f32: null pointer");
    ASR_REQUIRE(pixels > 0 && classes > 0 && (kind == 1 || kind == 2), "asr_class_activation_f32: bad arguments (kind 1 = softmax, 2 = sigmoid)");
    if (classes <= kMaxStageClasses)
        hipLaunchKernelGGL(class_activation_kernel<true>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out, pixels,
                           classes, kind);
    else
        hipLaunchKernelGGL(class_activation_kernel<false>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out,
                           pixels, classes, kind);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_opm_confidence_f32(const float* logits, float* out, int64_t pixels, int classes, int kind,
                                      asr_stream_t stream) {
    ASR_REQUIRE(logits && out, "asr_opm_confidence_f32: null pointer");
    ASR_REQUIRE(pixels > 0 && classes > 0, "asr_opm_confidence_f32: bad shape (pixels=%lld classes=%d)", (long long)pixels, classes);
    ASR_REQUIRE(kind == ASR_CONF_MAXPROB || kind == ASR_CONF_MARGIN, "asr_opm_confidence_f32: unknown kind %d (1 = maxprob, 2 = margin)", kind);
    if (classes > kMaxStageClasses)      // rows beyond the LDS tile: each thread walks its own row in global memory
        hipLaunchKernelGGL(opm_confidence_kernel<false>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out,
                           pixels, classes, kind);
    else
        hipLaunchKernelGGL(opm_confidence_kernel<true>, dim3(stream_grid(pixels)), dim3(256), 0, asr_stream(stream), logits, out, pixels,
                           classes, kind);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_boundary_dist2_u16(const int32_t* truth, uint16_t* dist2, int segments, int h, int w, int r_max,
                                      asr_stream_t stream) {
    ASR_REQUIRE(truth && dist2, "asr_boundary_dist2_u16: null pointer");
    ASR_REQUIRE(segments > 0 && segments <= 65535 && h >= 1 && w >= 1 && h <= (1 << 20) && w <= (1 << 20),
                "asr_boundary_dist2_u16: bad shape (segments=%d h=%d w=%d; 1..65535 segments, sides 1..2^20)", segments, h, w);
    ASR_REQUIRE(r_max >= 1 && r_max <= kDistMaxR, "asr_boundary_dist2_u16: r_max %d (1..%d)", r_max, kDistMaxR);
    hipLaunchKernelGGL(boundary_dist2_kernel, dim3((unsigned)asr_cdiv(w, 64), (unsigned)asr_cdiv(h, kDistRows), (unsigned)segments),
                       dim3(256), 0, asr_stream(stream), truth, dist2, h, w, r_max);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_band_class_counts_i32(const int32_t* truth, const int32_t* preds, const uint16_t* dist2, const int* widths,
                                         int64_t* counts, int64_t pixels, int num_preds, int num_widths, int r_max,
                                         int ignore_label, asr_stream_t stream) {
    ASR_REQUIRE(truth && preds && dist2 && counts, "asr_band_class_counts_i32: null pointer");
    ASR_REQUIRE(widths, "asr_band_class_counts_i32: null width array");
    ASR_REQUIRE(pixels > 0, "asr_band_class_counts_i32: bad shape (pixels=%lld)", (long long)pixels);
    ASR_REQUIRE(num_preds >= 1 && num_preds <= kBandMaxPreds, "asr_band_class_counts_i32: %d predictions (1..%d)", num_preds,
                kBandMaxPreds);
    ASR_REQUIRE(num_widths >= 1 && num_widths <= kBandMaxWidths, "asr_band_class_counts_i32: %d widths (1..%d)", num_widths,
                kBandMaxWidths);
    ASR_REQUIRE(r_max >= 1 && r_max <= kDistMaxR, "asr_band_class_counts_i32: r_max %d (1..%d)", r_max, kDistMaxR);
    AsrBandSet set = {};
    set.n = num_widths;
    for (int b = 0; b < num_widths; ++b) {
        ASR_REQUIRE(widths[b] >= 1 && widths[b] <= kDistMaxR, "asr_band_class_counts_i32: width %d out of range (1..%d)",
                    widths[b], kDistMaxR);
        ASR_REQUIRE(widths[b] <= r_max, "asr_band_class_counts_i32: width %d > r_max %d of the distance map", widths[b], r_max);
    }
    for (int v = 1; v <= kDistMaxR; ++v) {                      // the distinct widths, ascending
        bool used = false;
        for (int b = 0; b < num_widths; ++b)
            if (widths[b] == v) { set.slot[b] = set.u; used = true; }
        if (used) set.w2[set.u++] = v * v;
    }
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 768 * (size_t)num_preds * (size_t)num_widths, s));
    const int grid = stream_grid(pixels) > 64 ? 64 : stream_grid(pixels);
    hipLaunchKernelGGL(band_hist_kernel, dim3(grid, num_preds), dim3(256), sizeof(unsigned int) * 768 * (size_t)set.u, s, truth,
                       preds, dist2, reinterpret_cast<unsigned long long*>(counts), pixels, ignore_label, set);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(band_finalize_kernel, dim3((unsigned)asr_cdiv((int64_t)num_preds * 768, 256)), dim3(256), 0, s,
                       reinterpret_cast<long long*>(counts), num_preds, set);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_binned_class_counts_f32(const int32_t* truth, const int32_t* preds, const float* u, const float* edges,
                                           int64_t* counts, int64_t pixels, int num_preds, int num_bins, int ignore_label,
                                           asr_stream_t stream) {
    ASR_REQUIRE(truth && preds && u && edges && counts, "asr_binned_class_counts_f32: null pointer");
    ASR_REQUIRE(pixels > 0 && pixels < ((int64_t)1 << 62), "asr_binned_class_counts_f32: bad shape (pixels=%lld)", (long long)pixels);
    ASR_REQUIRE(num_preds >= 1 && num_preds <= kBinnedMaxPreds, "asr_binned_class_counts_f32: %d predictions (1..%d)", num_preds,
                kBinnedMaxPreds);
    ASR_REQUIRE(num_bins >= 1 && num_bins <= kBinnedMaxBins, "asr_binned_class_counts_f32: %d bins (1..%d)", num_bins,
                kBinnedMaxBins);
    // a workgroup's bins are 32-bit: with G workgroups in a grid row it sees fewer than pixels / G + 256 pixels, and
    // G >= pixels / 2^31 keeps that below 2^32 (asr_confusion_counts_i32's argument)
    int64_t grid = asr_cdiv(pixels, (int64_t)256);
    grid = grid > 64 ? 64 : grid;
    const int64_t need = asr_cdiv(pixels, (int64_t)1 << 31);
    grid = grid < need ? need : grid;
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 768 * (size_t)num_preds * (size_t)num_bins, s));
    hipLaunchKernelGGL(binned_hist_kernel, dim3((unsigned)grid, num_preds), dim3(256), sizeof(unsigned int) * 768 * (size_t)num_bins, s,
                       truth, preds, u, edges, reinterpret_cast<unsigned long long*>(counts), pixels, ignore_label, num_bins);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_confusion_counts_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels,
                                        int num_preds, int num_labels, asr_stream_t stream) {
    ASR_REQUIRE(truth && preds && counts, "asr_confusion_counts_i32: null pointer");
    ASR_REQUIRE(pixels > 0 && pixels < ((int64_t)1 << 62), "asr_confusion_counts_i32: bad shape (pixels=%lld)", (long long)pixels);
    ASR_REQUIRE(num_preds >= 1 && num_preds <= ASR_CONFUSION_MAX_PREDS, "asr_confusion_counts_i32: %d predictions (1..%d)",
                num_preds, ASR_CONFUSION_MAX_PREDS);
    ASR_REQUIRE(num_labels >= 1 && num_labels <= ASR_CONFUSION_MAX_LABELS, "asr_confusion_counts_i32: %d labels (1..%d)",
                num_labels, ASR_CONFUSION_MAX_LABELS);
    const size_t bins = (size_t)(num_labels + 1) * (size_t)(num_labels + 1);
    // A workgroup's bins are 32-bit: it must see fewer than 2^32 pixels.  With G workgroups in a grid row it makes
    // ceil(pixels / (G * span)) trips of span pixels, fewer than pixels / G + span; G >= pixels / 2^31 keeps that below
    // 2^31 + span.  Up to 2^37 pixels ASR_CONFUSION_GRID workgroups do; below 2^62 pixels G fits a grid dimension.
    int64_t grid = asr_cdiv(pixels, (int64_t)ASR_CONFUSION_SPAN);
    grid = grid > ASR_CONFUSION_GRID ? ASR_CONFUSION_GRID : grid;
    const int64_t need = asr_cdiv(pixels, (int64_t)1 << 31);
    grid = grid < need ? need : grid;
    hipStream_t s = asr_stream(stream);
    ASR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * bins * (size_t)num_preds, s));
    hipLaunchKernelGGL(confusion_hist_kernel, dim3((unsigned)grid, num_preds), dim3(256), sizeof(unsigned int) * bins, s, truth,
                       preds, reinterpret_cast<unsigned long long*>(counts), pixels, num_labels);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
