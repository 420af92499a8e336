// FreeU v2 on the two inputs of a UNet output block (include/fmx.h, section "FreeU v2"): backbone scaling by the normalised channel mean and the
// skip feature's four-bin Fourier filter in closed form.  Two HBM-bound passes: reduce reads h and skip once, apply reads them once more and
// writes half of h and all of skip.  fp16 storage, fp32 arithmetic, no floating-point atomics (partials are added in chunk order).
#include "fmx_common.hpp"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / FMX_WAVE;
constexpr int CP = FMX_FREEU_CHUNK_PIXELS;
constexpr int NB = 7;   // 1, cos tr, sin tr, cos tc, sin tc, cos(tr+tc), sin(tr+tc)

struct Workspace {
  float *mean, *minmax, *partial, *sums, *lohi;
};

inline Workspace carve(float* ws, long n, long hw, long cs, long nchunks) {
  Workspace w;
  w.mean = ws;
  w.minmax = w.mean + FMX_FREEU_PAD4(n * hw);
  w.partial = w.minmax + FMX_FREEU_PAD4(n * nchunks * 2);
  w.sums = w.partial + n * nchunks * NB * cs;
  w.lohi = w.sums + n * NB * cs;
  return w;
}

// the seven basis values of pixel p from the host's tables (cos tr | sin tr | cos tc | sin tc)
__device__ __forceinline__ void basis_of(const float* __restrict__ trig, int hh, int ww, int p, float (&bs)[NB]) {
  const int r = p / ww, c = p - r * ww;
  const float cr = trig[r], sr = trig[hh + r], cc = trig[2 * hh + c], sc = trig[2 * hh + ww + c];
  bs[0] = 1.0f;
  bs[1] = cr;
  bs[2] = sr;
  bs[3] = cc;
  bs[4] = sc;
  bs[5] = cr * cc - sr * sc;
  bs[6] = sr * cc + cr * sc;
}

// how the TPB threads of a workgroup share `gper` 8-channel groups of skip: `nsub` threads per group, each taking every nsub-th pixel of the chunk
struct SkipMap {
  int gper, nsub, sub, gl;
  bool active;
  __device__ SkipMap(int ncg, int g0) {
    gper = min(TPB, ncg - g0);
    nsub = TPB / gper;
    sub = (int)threadIdx.x / gper;
    gl = (int)threadIdx.x - sub * gper;
    active = sub < nsub;
  }
};

__device__ __forceinline__ float sum8(const f16x8 v) {
  float a = (float)v[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) a += (float)v[j];
  return a;
}

// grid (nchunks, n).  From h: the channel mean of every pixel of the chunk (one wave per pixel, lanes over 16-byte vectors, xor-butterfly sum) and
// the chunk's min / max of it.  From skip: the seven weighted sums of the chunk per channel (a thread keeps 8 channels x 7 sums, the threads that
// share a channel group are added through LDS in thread order).
__global__ __launch_bounds__(TPB) void freeu_reduce_kernel(const f16* __restrict__ h, int ch, const f16* __restrict__ skip, int cs, int hh, int ww,
                                                           const float* __restrict__ trig, int nchunks, Workspace w) {
  const int chunk = blockIdx.x, n = blockIdx.y, hw = hh * ww;
  const int start = chunk * CP, cnt = min(CP, hw - start);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float red[2 * WAVES];
  __shared__ __attribute__((aligned(16))) float fold[TPB * 8];

  {
    const int nv = ch / 8;
    const float inv_c = 1.0f / (float)ch;
    float lo = INFINITY, hi = -INFINITY;
    for (int pi = wave; pi < cnt; pi += 2 * WAVES) {
      const int pj = pi + WAVES;
      const bool two = pj < cnt;
      const f16x8* r0 = reinterpret_cast<const f16x8*>(h + ((size_t)n * hw + start + pi) * ch);
      const f16x8* r1 = reinterpret_cast<const f16x8*>(h + ((size_t)n * hw + start + (two ? pj : pi)) * ch);
      float a0 = 0.f, a1 = 0.f;
      for (int v = lane; v < nv; v += FMX_WAVE) {
        a0 += sum8(r0[v]);
        a1 += sum8(r1[v]);
      }
      const float m0 = wave_sum(a0) * inv_c, m1 = wave_sum(a1) * inv_c;
      lo = fminf(lo, m0);
      hi = fmaxf(hi, m0);
      if (two) {
        lo = fminf(lo, m1);
        hi = fmaxf(hi, m1);
      }
      if (lane == 0) {
        w.mean[(size_t)n * hw + start + pi] = m0;
        if (two) w.mean[(size_t)n * hw + start + pj] = m1;
      }
    }
    if (lane == 0) {
      red[wave] = lo;
      red[WAVES + wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < WAVES; ++k) {
        lo = fminf(lo, red[k]);
        hi = fmaxf(hi, red[WAVES + k]);
      }
      w.minmax[((size_t)n * nchunks + chunk) * 2] = lo;
      w.minmax[((size_t)n * nchunks + chunk) * 2 + 1] = hi;
    }
  }

  const int ncg = cs / 8;
  for (int g0 = 0; g0 < ncg; g0 += TPB) {
    const SkipMap mp(ncg, g0);
    float acc[NB][8];
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    if (mp.active) {
      const f16* base = skip + ((size_t)n * hw + start) * cs + (size_t)(g0 + mp.gl) * 8;
      for (int pi = mp.sub; pi < cnt; pi += mp.nsub) {
        float bs[NB];
        basis_of(trig, hh, ww, start + pi, bs);
        const f16x8 v = *reinterpret_cast<const f16x8*>(base + (size_t)pi * cs);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = (float)v[j];
#pragma unroll
          for (int k = 0; k < NB; ++k) acc[k][j] += x * bs[k];
        }
      }
    }
    float* dst = w.partial + ((size_t)n * nchunks + chunk) * NB * cs + (size_t)(g0 + mp.gl) * 8;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      __syncthreads();
      if (mp.active) {
#pragma unroll
        for (int j = 0; j < 8; ++j) fold[(mp.sub * mp.gper + mp.gl) * 8 + j] = acc[k][j];
      }
      __syncthreads();
      if (mp.sub == 0) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = acc[k][j];
        for (int s = 1; s < mp.nsub; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) t[j] += fold[(s * mp.gper + mp.gl) * 8 + j];
        *reinterpret_cast<f32x4*>(dst + (size_t)k * cs) = f32x4{t[0], t[1], t[2], t[3]};
        *reinterpret_cast<f32x4*>(dst + (size_t)k * cs + 4) = f32x4{t[4], t[5], t[6], t[7]};
      }
    }
  }
}

// grid (ceil(7*cs / TPB), n): sums[n][k][c] = the chunks' partials added in chunk order; the first workgroup of a sample also folds lo / hi
// (min and max are exact, their order does not matter)
__global__ __launch_bounds__(TPB) void freeu_fold_kernel(int cs, int nchunks, Workspace w) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < NB * cs) {
    const float* src = w.partial + (size_t)n * nchunks * NB * cs + i;
    float t = 0.f;
    for (int c = 0; c < nchunks; ++c) t += src[(size_t)c * NB * cs];
    w.sums[(size_t)n * NB * cs + i] = t;
  }
  if (blockIdx.x == 0) {
    __shared__ float red[2 * WAVES];
    float lo = INFINITY, hi = -INFINITY;
    for (int c = threadIdx.x; c < nchunks; c += TPB) {
      lo = fminf(lo, w.minmax[((size_t)n * nchunks + c) * 2]);
      hi = fmaxf(hi, w.minmax[((size_t)n * nchunks + c) * 2 + 1]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6] = lo;
      red[WAVES + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < WAVES; ++k) {
        lo = fminf(lo, red[k]);
        hi = fmaxf(hi, red[WAVES + k]);
      }
      w.lohi[n * 2] = lo;
      w.lohi[n * 2 + 1] = hi;
    }
  }
}

// grid (nchunks, n), in place: the first half of h's channels times the backbone factor of their pixel, skip plus the scaled low-frequency part
__global__ __launch_bounds__(TPB) void freeu_apply_kernel(f16* h, int ch, f16* skip, int cs, int hh, int ww, const float* __restrict__ trig,
                                                          Workspace w, float bm1, float coef) {
  const int chunk = blockIdx.x, n = blockIdx.y, hw = hh * ww;
  const int start = chunk * CP, cnt = min(CP, hw - start);

  {
    const float lo = w.lohi[n * 2], hi = w.lohi[n * 2 + 1];
    const float range = hi - lo;
    const int nv = ch / 16;                      // 16-byte vectors in the scaled half of a pixel
    for (int i = threadIdx.x; i < cnt * nv; i += TPB) {
      const int pi = i / nv, v = i - pi * nv;
      const float m = w.mean[(size_t)n * hw + start + pi];
      const float g = bm1 * ((m - lo) / range) + 1.0f;
      f16x8* ptr = reinterpret_cast<f16x8*>(h + ((size_t)n * hw + start + pi) * ch) + v;
      f16x8 x = *ptr;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (f16)((float)x[j] * g);
      *ptr = x;
    }
  }

  const int ncg = cs / 8;
  for (int g0 = 0; g0 < ncg; g0 += TPB) {
    const SkipMap mp(ncg, g0);
    if (!mp.active) continue;
    float sk[NB][8];
    const float* src = w.sums + (size_t)n * NB * cs + (size_t)(g0 + mp.gl) * 8;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)k * cs), b = *reinterpret_cast<const f32x4*>(src + (size_t)k * cs + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sk[k][j] = a[j];
        sk[k][4 + j] = b[j];
      }
    }
    f16* base = skip + ((size_t)n * hw + start) * cs + (size_t)(g0 + mp.gl) * 8;
    for (int pi = mp.sub; pi < cnt; pi += mp.nsub) {
      float bs[NB];
      basis_of(trig, hh, ww, start + pi, bs);
      f16x8* ptr = reinterpret_cast<f16x8*>(base + (size_t)pi * cs);
      f16x8 x = *ptr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float low = sk[0][j];
#pragma unroll
        for (int k = 1; k < NB; ++k) low += sk[k][j] * bs[k];
        x[j] = (f16)((float)x[j] + coef * low);
      }
      *ptr = x;
    }
  }
}

int check_args(const char* who, const void* h, int32_t c_h, const void* skip, int32_t c_s, int32_t n, int32_t hh, int32_t ww, const float* trig,
               int32_t nchunks, const float* workspace, int64_t workspace_floats) {
  FMX_REQUIRE(h && skip && trig && workspace, "%s: null pointer", who);
  FMX_REQUIRE(fmx_aligned16(h) && fmx_aligned16(skip) && fmx_aligned16(trig) && fmx_aligned16(workspace), "%s: pointers must be 16-byte aligned", who);
  FMX_REQUIRE(n > 0 && n <= 65535 && hh > 0 && ww > 0 && c_h > 0 && c_s > 0, "%s: bad dims n=%d hh=%d ww=%d c_h=%d c_s=%d", who, n, hh, ww, c_h, c_s);
  FMX_REQUIRE(hh >= 2 && ww >= 2, "%s: the Fourier filter is defined for H >= 2 and W >= 2 only, got %d x %d", who, hh, ww);
  FMX_REQUIRE((c_h % 16) == 0 && (c_s % 8) == 0, "%s: c_h must be a multiple of 16 and c_s a multiple of 8, got %d / %d", who, c_h, c_s);
  const int64_t hw = (int64_t)hh * ww;
  FMX_REQUIRE(hw < (1LL << 31), "%s: %d x %d pixels per sample are out of range", who, hh, ww);
  FMX_REQUIRE(nchunks == (hw + CP - 1) / CP, "%s: nchunks must be ceil(hh*ww / %d) = %lld, got %d", who, CP, (long long)((hw + CP - 1) / CP), nchunks);
  const int64_t need = FMX_FREEU_WORKSPACE_FLOATS(n, hw, c_s, nchunks);
  FMX_REQUIRE(workspace_floats >= need, "%s: workspace of %lld floats, %lld needed for %d chunks", who, (long long)workspace_floats, (long long)need,
              nchunks);
  return 0;
}

}  // namespace

extern "C" int fmx_freeu_reduce_f16(const void* h, int32_t c_h, const void* skip, int32_t c_s, int32_t n, int32_t hh, int32_t ww, const float* trig,
                                    int32_t nchunks, float* workspace, int64_t workspace_floats, void* stream) {
  if (int rc = check_args("freeu_reduce", h, c_h, skip, c_s, n, hh, ww, trig, nchunks, workspace, workspace_floats)) return rc;
  const Workspace w = carve(workspace, n, (long)hh * ww, c_s, nchunks);
  hipLaunchKernelGGL(freeu_reduce_kernel, dim3(nchunks, n), dim3(TPB), 0, (hipStream_t)stream, (const f16*)h, c_h, (const f16*)skip, c_s, hh, ww, trig,
                     nchunks, w);
  FMX_LAUNCH_CHECK("fmx_freeu_reduce_f16");
  return 0;
}

extern "C" int fmx_freeu_apply_f16(void* h, int32_t c_h, void* skip, int32_t c_s, int32_t n, int32_t hh, int32_t ww, const float* trig, int32_t nchunks,
                                   float* workspace, int64_t workspace_floats, float b, float s, void* stream) {
  if (int rc = check_args("freeu_apply", h, c_h, skip, c_s, n, hh, ww, trig, nchunks, workspace, workspace_floats)) return rc;
  const Workspace w = carve(workspace, n, (long)hh * ww, c_s, nchunks);
  hipLaunchKernelGGL(freeu_fold_kernel, dim3((NB * c_s + TPB - 1) / TPB, n), dim3(TPB), 0, (hipStream_t)stream, c_s, nchunks, w);
  FMX_LAUNCH_CHECK("fmx_freeu_apply_f16 (fold)");
  hipLaunchKernelGGL(freeu_apply_kernel, dim3(nchunks, n), dim3(TPB), 0, (hipStream_t)stream, (f16*)h, c_h, (f16*)skip, c_s, hh, ww, trig, w, b - 1.0f,
                     (s - 1.0f) / ((float)hh * (float)ww));
  FMX_LAUNCH_CHECK("fmx_freeu_apply_f16");
  return 0;
}
