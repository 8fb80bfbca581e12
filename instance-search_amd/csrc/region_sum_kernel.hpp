// region_sum_kernel.hpp -- the TRAINING form of the region descriptor's first step (reference model/siamese.py:191-219 under autograd): for
// every image the k selected windows are gathered, L2-normalised, shifted and SUMMED into one row (the Linear behind it is linear, so it
// needs the sum alone), and the backward pass of exactly that.  Included by region.hip only; needs block_sum<NT> (isx_common.hpp).
//
// Layouts: fmap / dfmap / add (B,Hf,Wf,C) channels-last; rows / g (B,F), F = C*kh*kw in the Linear's (c, a, b) column order; flat_idx (B,k)
// as isx_region_topk_nhwc writes it (row = fi / Wp, col = fi % Wp); n2 / cw (B,k).  An entry fi outside [0, Hp*Wp) is SKIPPED.
//
// Orders (include/isx.h states them, tests/_region_train_model.py restates them):
//   window sums   ss_w = sum v^2 and c_w = sum v g over the window in its (a, b, c) order, the order of region_gather_l2_nhwc_kernel: thread t of
//                 1024 owns the float4 groups t, t + 1024, ... and adds the four products of each to its accumulator one by one, from +0; the
//                 butterfly in every wave, the 16 wave sums in order (block_sum<1024>).  A function of the window alone.
//   rows          t_w = v / sqrtf(n2_w) + (shift ? shift[j] : 0), rows = ((t_0 + t_1) + ...) over the valid windows in ascending w.
//   dfmap         acc = +0; acc += (n2_w g - v c_w) * inv_w over the valid windows that cover the pixel, ascending w; then + add (the images
//                 that have one: every add_every-th).
#pragma once

namespace isx {

__device__ __forceinline__ bool region_window_valid(int64_t fi, int Hp, int Wp) { return fi >= 0 && fi < (int64_t)Hp * Wp; }

// One 1024-thread block per (window, image).  DOT = false: out = ss + eps (n2); DOT = true: out = sum v g (c_w).  A skipped entry writes +0.
template <bool DOT>
__global__ __launch_bounds__(1024) void region_window_stat_kernel(const float* __restrict__ fmap_all, const float* __restrict__ g_all, int C, int Hf,
                                                                  int Wf, int kh, int kw, const int64_t* __restrict__ flat_idx, int Wp, float eps,
                                                                  float* __restrict__ out) {
    __shared__ float red[16];
    const int khw = kh * kw, C4 = C >> 2;
    const int run4 = kw * C4;                                   // float4 per window row
    const int F4 = kh * run4;
    const int64_t w = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t fi = flat_idx[w];
    if (!region_window_valid(fi, Hf - kh + 1, Wp)) {
        if (threadIdx.x == 0) out[w] = 0.0f;
        return;
    }
    const int row = (int)(fi / Wp), col = (int)(fi % Wp);
    const float* base = fmap_all + ((int64_t)blockIdx.y * Hf * Wf + (int64_t)row * Wf + col) * C;
    const float* g = DOT ? g_all + (int64_t)blockIdx.y * C * khw : nullptr;
    float acc = 0.0f;
    for (int j = threadIdx.x; j < F4; j += 1024) {
        const int a = j / run4, r = j - a * run4;
        const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)a * Wf * C + r * 4);
        if (DOT) {
            const int b = r / C4, c = (r - b * C4) * 4;
            const float* gj = g + (int64_t)c * khw + a * kw + b;
            acc += v.x * gj[0]; acc += v.y * gj[khw]; acc += v.z * gj[2 * khw]; acc += v.w * gj[3 * khw];
        } else {
            acc += v.x * v.x; acc += v.y * v.y; acc += v.z * v.z; acc += v.w * v.w;
        }
    }
    acc = block_sum<1024>(acc, red);
    if (threadIdx.x == 0) out[w] = DOT ? acc : acc + eps;
}

// One 256-thread block per (slice of CS channels, image).  The slice of the whole map is staged in LDS (16-B loads of consecutive lanes; pixel
// stride CS + 1 floats, so that the (c, a, b)-ordered reads below fall on distinct banks), then the block writes its contiguous run of cs*kh*kw
// floats of the image's row.  LDS: Hf*Wf*(CS+1) floats, then k floats (sqrtf(n2_w)) and k ints (window's first pixel, -1: skipped).
__global__ __launch_bounds__(256) void region_sum_l2_nhwc_kernel(const float* __restrict__ fmap_all, int C, int Hf, int Wf, int kh, int kw,
                                                                 const int64_t* __restrict__ flat_idx, int k, int Wp,
                                                                 const float* __restrict__ shift, const float* __restrict__ n2, int CS,
                                                                 float* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int HW = Hf * Wf, LS = CS + 1, khw = kh * kw;
    const int c0 = blockIdx.x * CS;
    const int cs = C - c0 < CS ? C - c0 : CS;
    float* wn = lds + HW * LS;
    int* wpos = reinterpret_cast<int*>(wn + k);
    for (int i = threadIdx.x; i < k; i += 256) {
        const int64_t fi = flat_idx[(int64_t)blockIdx.y * k + i];
        const bool ok = region_window_valid(fi, Hf - kh + 1, Wp);
        wpos[i] = ok ? (int)(fi / Wp) * Wf + (int)(fi % Wp) : -1;
        wn[i] = ok ? sqrtf(n2[(int64_t)blockIdx.y * k + i]) : 1.0f;
    }
    const int q4 = cs >> 2;
    const float* src = fmap_all + (int64_t)blockIdx.y * HW * C + c0;
    for (int i = threadIdx.x; i < HW * q4; i += 256) {
        const int p = i / q4, cq = i - p * q4;
        const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)p * C + cq * 4);
        float* l = lds + p * LS + cq * 4;
        l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
    }
    __syncthreads();
    const int n = cs * khw;
    float* out = rows + ((int64_t)blockIdx.y * C + c0) * khw;
    const float* sh = shift ? shift + (int64_t)c0 * khw : nullptr;
    for (int j = threadIdx.x; j < n; j += 256) {
        const int c = j / khw, r = j - c * khw, a = r / kw, b = r - a * kw;
        const int off = (a * Wf + b) * LS + c;
        const float s = sh ? sh[j] : 0.0f;
        float acc = 0.0f;
        bool first = true;
        for (int w = 0; w < k; ++w) {
            const int p = wpos[w];
            if (p < 0) continue;
            const float t = lds[p * LS + off] / wn[w] + s;
            acc = first ? t : acc + t;
            first = false;
        }
        out[j] = acc;
    }
}

// One 256-thread block per (slice of CS channels, image), gather form: the slice's contiguous run of cs*kh*kw floats of g is staged in LDS, a
// thread owns 4 consecutive channels of a map pixel (its own v) and adds the windows that cover the pixel in ascending w.  LDS: CS*kh*kw floats,
// then per window n2, c_w, inv (floats) and row, col (ints; row -1: skipped).
__global__ __launch_bounds__(256) void region_sum_l2_bwd_nhwc_kernel(const float* __restrict__ fmap_all, const float* __restrict__ g_all,
                                                                     const float* __restrict__ n2, const float* __restrict__ cw, int C, int Hf,
                                                                     int Wf, int kh, int kw, const int64_t* __restrict__ flat_idx, int k, int Wp,
                                                                     const float* __restrict__ add_all, int add_every, int CS, float* __restrict__ dfmap_all) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int HW = Hf * Wf, khw = kh * kw;
    const int c0 = blockIdx.x * CS;
    const int cs = C - c0 < CS ? C - c0 : CS;
    float* wn2 = lds + CS * khw;
    float* wc = wn2 + k;
    float* winv = wc + k;
    int* wrow = reinterpret_cast<int*>(winv + k);
    int* wcol = wrow + k;
    for (int i = threadIdx.x; i < k; i += 256) {
        const int64_t fi = flat_idx[(int64_t)blockIdx.y * k + i];
        const bool ok = region_window_valid(fi, Hf - kh + 1, Wp);
        const float v2 = ok ? n2[(int64_t)blockIdx.y * k + i] : 1.0f;
        wrow[i] = ok ? (int)(fi / Wp) : -1;
        wcol[i] = ok ? (int)(fi % Wp) : 0;
        wn2[i] = v2;
        wc[i] = ok ? cw[(int64_t)blockIdx.y * k + i] : 0.0f;
        winv[i] = 1.0f / (v2 * sqrtf(v2));
    }
    const int n4 = (cs * khw) >> 2;
    const float4* gsrc = reinterpret_cast<const float4*>(g_all + ((int64_t)blockIdx.y * C + c0) * khw);
    float4* l4 = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < n4; i += 256) l4[i] = gsrc[i];
    __syncthreads();
    const int q4 = cs >> 2;
    const int64_t img = (int64_t)blockIdx.y * HW * C + c0;
    // add holds one map per add_every images: image b takes map b / add_every when b % add_every == 0, the others take none
    const float* add = add_all && blockIdx.y % add_every == 0 ? add_all + (int64_t)(blockIdx.y / add_every) * HW * C + c0 : nullptr;
    for (int o = threadIdx.x; o < HW * q4; o += 256) {
        const int pix = o / q4, cq = o - pix * q4, y = pix / Wf, x = pix - y * Wf;
        const int64_t at = img + (int64_t)pix * C + cq * 4;
        const float4 v = *reinterpret_cast<const float4*>(fmap_all + at);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int w = 0; w < k; ++w) {
            const int a = y - wrow[w], b = x - wcol[w];
            if (wrow[w] < 0 || a < 0 || a >= kh || b < 0 || b >= kw) continue;
            const float* gl = lds + cq * 4 * khw + a * kw + b;
            const float m = wn2[w], cc = wc[w], inv = winv[w];
            s.x += (m * gl[0] - v.x * cc) * inv;
            s.y += (m * gl[khw] - v.y * cc) * inv;
            s.z += (m * gl[2 * khw] - v.z * cc) * inv;
            s.w += (m * gl[3 * khw] - v.w * cc) * inv;
        }
        if (add) {
            const float4 e = *reinterpret_cast<const float4*>(add + (int64_t)pix * C + cq * 4);
            s.x += e.x; s.y += e.y; s.z += e.z; s.w += e.w;
        }
        *reinterpret_cast<float4*>(dfmap_all + at) = s;
    }
}

// Largest channel slice (64, 32, ..., 4) whose LDS need, per_channel * CS + fixed floats, stays within 64 KB; 0: none does.
inline int region_slice(int64_t per_channel, int64_t fixed) {
    for (int cs = 64; cs >= 4; cs >>= 1)
        if ((per_channel * cs + fixed) * 4 <= 64 * 1024) return cs;
    return 0;
}

}  // namespace isx
