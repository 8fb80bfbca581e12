// augment.hip -- training-time augmentation of the reference (utils/image.py:128-187, random_affine_noisy_cv): an affine warp through cubic
// B-spline interpolation (scipy.ndimage.affine_transform, order 3, mode 'constant'), the reference's wrap-around uint8 cast, random bytes
// where the warp leaves the input, and ToTensor + Normalize -- one entry, isx_affine_noisy_u8, three launches:
//
//   spline_columns_kernel   uint8 pixels (through `rows`) -> fp64, recursive filter along axis 0.  One thread per (image, x, channel) column;
//                           the workspace is (B,H,W,3) fp64, so the 3W threads of an image row read and write consecutive addresses.
//   spline_rows_kernel      the same filter along axis 1.  A workgroup stages R whole image rows (one contiguous stretch of the workspace) in
//                           LDS, 3R threads run the recursion on LDS lines of stride 3, all threads copy the tile back.  The LDS row stride
//                           is padded to 3 (mod 32) doubles: line (r, c) then starts in 8-byte bank 3r + c, conflict-free for up to 10 rows.
//   warp_noise_kernel       one thread per output pixel: coordinates, 4 x 4 taps x 3 channels (a tap's channels are 24 contiguous bytes),
//                           cast, noise, both outputs.
//
// All of it in fp64 with ONE rounding per operation: `#pragma clang fp contract(off)` below (and -ffp-contract=off on the command line), plain
// IEEE division; the operation order is the one tests/_augment_model.py and utils/image.py restate in numpy.
#include "isx_common.hpp"

#pragma clang fp contract(off)

namespace isx {

namespace {

constexpr int kRowThreads = 256;
constexpr int kMaxRowTile = 10;                       // image rows per workgroup of spline_rows_kernel (bank layout above)
constexpr size_t kRowLdsBudget = 64 * 1024;

struct Pole {
    double z, gain, last;                             // z = sqrt(3) - 2, (1 - z)(1 - 1/z), z / (z^2 - 1)
};
__device__ __forceinline__ Pole pole() {
    const double z = sqrt(3.0) - 2.0;
    return {z, (1.0 - z) * (1.0 - 1.0 / z), z / (z * z - 1.0)};
}

__device__ __forceinline__ double pow_chain(double z, int k) {          // z^k as k multiplications from 1.0 (what the model does)
    double p = 1.0;
    for (int i = 0; i < k; ++i) p = p * z;
    return p;
}

// The recursive filter on one line of n >= 2 values: in(i) is input element i times the gain, at(i) a reference to where coefficient i lives
// (the two may be the same storage: element i is read before it is written).  The passes move in chunks of 8 elements -- 8 independent loads
// in flight, then the dependent chain -- because the chain alone would expose one memory latency per element.
template <typename In, typename At>
__device__ __forceinline__ void filter_line(In in, At at, int n, const Pole& P) {
    const double z = P.z;
    const double zn1 = pow_chain(z, n - 1);
    double c0 = in(0) + zn1 * in(n - 1);
    double zi = z;
    for (int i = 1; i <= n - 2 && fabs(zi) >= 1e-30; ++i) {
        c0 = c0 + zi * (in(i) + zn1 * in(n - 1 - i));
        zi = zi * z;
    }
    double prev = c0 / (1.0 - zn1 * zn1);
    double before_last = prev;                        // coefficient n - 2 of the causal pass
    double v[8];
    for (int i0 = 1; i0 < n; i0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = i0 + k < n ? in(i0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + k < n) {
                before_last = prev;
                prev = v[k] + z * prev;
                at(i0 + k) = prev;
            }
        }
    }
    at(0) = c0 / (1.0 - zn1 * zn1);
    prev = (z * before_last + prev) * P.last;
    at(n - 1) = prev;
    for (int i0 = n - 2; i0 >= 0; i0 -= 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = i0 - k >= 0 ? at(i0 - k) : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 - k >= 0) {
                prev = z * (prev - v[k]);
                at(i0 - k) = prev;
            }
        }
    }
}

__global__ __launch_bounds__(128) void spline_columns_kernel(const uint8_t* __restrict__ img, const int64_t* __restrict__ rows, int H, int W,
                                                             double* __restrict__ ws) {
    const int t = blockIdx.x * 128 + threadIdx.x;      // x * 3 + c
    if (t >= 3 * W) return;
    const int64_t b = blockIdx.y;
    const int64_t stride = 3 * (int64_t)W;
    const uint8_t* src = img + (rows ? rows[b] : b) * stride * H + t;
    double* dst = ws + b * stride * H + t;
    const Pole P = pole();
    if (H == 1) {
        dst[0] = (double)src[0];
        return;
    }
    filter_line([&](int i) { return (double)src[i * stride] * P.gain; }, [&](int i) -> double& { return dst[i * stride]; }, H, P);
}

__global__ __launch_bounds__(kRowThreads) void spline_rows_kernel(double* __restrict__ ws, int H, int W, int R, int lds_stride) {
    extern __shared__ double tile[];
    const int64_t b = blockIdx.y;
    const int y0 = blockIdx.x * R;
    const int nrow = min(R, H - y0);
    const int row_len = 3 * W;
    double* base = ws + (b * H + y0) * (int64_t)row_len;
    const int total = nrow * row_len;
    for (int i = threadIdx.x; i < total; i += kRowThreads) {
        const int r = i / row_len;
        tile[r * lds_stride + (i - r * row_len)] = base[i];
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * nrow) {
        const Pole P = pole();
        double* line = tile + (threadIdx.x / 3) * lds_stride + (threadIdx.x % 3);
        filter_line([&](int i) { return line[3 * i] * P.gain; }, [&](int i) -> double& { return line[3 * i]; }, W, P);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += kRowThreads) {
        const int r = i / row_len;
        base[i] = tile[r * lds_stride + (i - r * row_len)];
    }
}

__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ __forceinline__ void spline_weights(double t, double* w) {
    const double u = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = u * u * u / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}

__device__ __forceinline__ uint8_t noise_byte(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint8_t)(z >> 56);
}

__global__ __launch_bounds__(256) void warp_noise_kernel(const double* __restrict__ ws, int64_t B, int H, int W, const double* __restrict__ mat,
                                                         uint64_t seed, const int64_t* __restrict__ noise_ids, const float* __restrict__ mean,
                                                         const float* __restrict__ sd, int nhwc, uint8_t* __restrict__ out_u8,
                                                         float* __restrict__ out_f32) {
    const int64_t HW = (int64_t)H * W, total = B * HW;
    float m[3] = {0.0f, 0.0f, 0.0f}, s[3] = {1.0f, 1.0f, 1.0f};
    if (mean) { m[0] = mean[0]; m[1] = mean[1]; m[2] = mean[2]; }
    if (sd) { s[0] = sd[0]; s[1] = sd[1]; s[2] = sd[2]; }
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        const int64_t b = p / HW;
        const int hw = (int)(p - b * HW);
        const int y = hw / W, x = hw - y * W;
        const double* M = mat + b * 6;
        const double yi = M[2] + M[0] * (double)y + M[1] * (double)x;
        const double xi = M[5] + M[3] * (double)y + M[4] * (double)x;
        uint8_t u[3];
        if (yi < 0.0 || yi > (double)(H - 1) || xi < 0.0 || xi > (double)(W - 1) || yi != yi || xi != xi) {
            const uint64_t counter = (uint64_t)noise_ids[b] * (uint64_t)(3 * HW) + (uint64_t)(3 * (int64_t)hw);
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = noise_byte(seed, counter + (uint64_t)c);
        } else {
            const double fy = floor(yi), fx = floor(xi);
            double wy[4], wx[4];
            spline_weights(yi - fy, wy);
            spline_weights(xi - fx, wx);
            int ix[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) ix[k] = 3 * mirror_index((int)fx + k - 1, W);
            const double* cb = ws + b * 3 * HW;
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* crow = cb + (int64_t)mirror_index((int)fy + j - 1, H) * (3 * W);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + crow[ix[k] + c] * wy[j] * wx[k];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = (uint8_t)((long long)acc[c] & 255);        // truncate toward zero, then modulo 256
        }
        if (out_u8) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out_u8[p * 3 + c] = u[c];
        }
        if (out_f32) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = ((float)u[c] / 255.0f - m[c]) / s[c];                     // the expression of images_u8_to_f32_kernel (pool.hip)
                if (nhwc) out_f32[p * 3 + c] = v;
                else out_f32[(b * 3 + c) * HW + hw] = v;
            }
        }
    }
}

// Rows per workgroup and LDS row stride (doubles) of spline_rows_kernel for images W wide; 0 rows = W does not fit.
void row_tile(int W, int* R, int* lds_stride) {
    const int row_len = 3 * W;
    *lds_stride = row_len + ((3 - row_len % 32) + 32) % 32;
    const size_t per_row = (size_t)*lds_stride * sizeof(double);
    const size_t fit = kRowLdsBudget / per_row;
    *R = (int)(fit < (size_t)kMaxRowTile ? fit : (size_t)kMaxRowTile);
}

}  // namespace

}  // namespace isx

ISX_API size_t isx_affine_noisy_workspace(int64_t B, int H, int W) {
    int R = 0, lds_stride = 0;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (int64_t)H * W * 3 >= (1ll << 31)) return 0;       // what isx_affine_noisy_u8 refuses (B = 0 needs none)
    isx::row_tile(W, &R, &lds_stride);
    if (R < 1) return 0;
    const size_t bytes = (size_t)B * 3 * (size_t)H * (size_t)W * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

ISX_API int isx_affine_noisy_u8(const uint8_t* img, const int64_t* rows, int64_t B, int H, int W, const double* mat, uint64_t seed,
                                const int64_t* noise_ids, const float* mean, const float* std, int channels_last, uint8_t* out_u8, float* out_f32,
                                void* ws, size_t ws_bytes, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31) && B <= 65535,
                "isx_affine_noisy_u8: bad shape B=%lld H=%d W=%d (B <= 65535, 3 H W < 2^31)", (long long)B, H, W);
    if (B == 0) return ISX_OK;
    int R = 0, lds_stride = 0;
    isx::row_tile(W, &R, &lds_stride);
    ISX_REQUIRE(R >= 1, "isx_affine_noisy_u8: W=%d too wide (one row of 3 W fp64 values has to fit 64 KiB of LDS)", W);
    ISX_REQUIRE(img && mat && noise_ids && ws && (out_u8 || out_f32), "isx_affine_noisy_u8: null pointer (img, mat, noise_ids, ws, and one of out_u8 / out_f32)");
    ISX_REQUIRE((((uintptr_t)ws | (uintptr_t)out_f32) % 16) == 0, "isx_affine_noisy_u8: ws and out_f32 must be 16-B aligned");
    ISX_REQUIRE((((uintptr_t)mat | (uintptr_t)noise_ids | (uintptr_t)rows) % 8) == 0 && (((uintptr_t)mean | (uintptr_t)std) % 4) == 0,
                "isx_affine_noisy_u8: mat, noise_ids and rows must be 8-B aligned, mean and std 4-B aligned");
    const size_t need = isx_affine_noisy_workspace(B, H, W);
    if (ws_bytes < need) {
        isx_set_error("isx_affine_noisy_u8: workspace too small: %zu bytes given, %zu needed", ws_bytes, need);
        return ISX_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double* coeff = static_cast<double*>(ws);
    hipLaunchKernelGGL(isx::spline_columns_kernel, dim3((unsigned)((3 * W + 127) / 128), (unsigned)B), dim3(128), 0, st, img, rows, H, W, coeff);
    ISX_CHECK_LAUNCH("isx_affine_noisy_u8 (columns)");
    if (W > 1) {
        hipLaunchKernelGGL(isx::spline_rows_kernel, dim3((unsigned)((H + R - 1) / R), (unsigned)B), dim3(isx::kRowThreads),
                           (size_t)R * lds_stride * sizeof(double), st, coeff, H, W, R, lds_stride);
        ISX_CHECK_LAUNCH("isx_affine_noisy_u8 (rows)");
    }
    const int64_t blocks = (B * H * W + 255) / 256;
    hipLaunchKernelGGL(isx::warp_noise_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, st, coeff, B, H, W, mat, seed,
                       noise_ids, mean, std, channels_last ? 1 : 0, out_u8, out_f32);
    ISX_CHECK_LAUNCH("isx_affine_noisy_u8 (warp)");
    return ISX_OK;
}
