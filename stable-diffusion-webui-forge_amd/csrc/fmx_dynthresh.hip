// Dynamic Thresholding (CFG-Fix) on the two denoised predictions of a step (include/fmx.h, section "Dynamic Thresholding"): an exact
// order-statistic selection over rows of fp32 values -- a most-significant-digit radix selection on the bit patterns, no sort -- and the
// three passes of the op itself (partial sums, scale references, apply).  fp32 throughout; integer LDS atomics only, whose result does not
// depend on their order; float sums are block reductions of a fixed shape.
#include "fmx_common.hpp"

// one rounding per operation, in the reference's order: the quantile has to see the very values the apply pass forms again
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;                      // partial-sum and apply passes
constexpr int CHUNK = FMX_DYNTHRESH_CHUNK;    // values of one row per workgroup in those passes
constexpr int SEL_TPB = 1024;                 // selection / reference pass: one workgroup per group of rows
constexpr int SEL_WAVES = SEL_TPB / FMX_WAVE;
constexpr int SEL_BINS = 2048;

struct SelShared {
  uint32_t hist[SEL_BINS];
  uint32_t prefix, k, cnt, ext;
  float red[2 * SEL_WAVES];
};

// ---- the values a selection runs over: functors with row(r) -> accessor(i) -> a non-negative float ------------------------------------------
struct AbsDiffRow {
  const float* x;
  float c;
  __device__ __forceinline__ float operator()(int64_t i) const { return fabsf(x[i] - c); }
};
struct AbsDiff {
  const float *x, *center;
  int n;
  __device__ __forceinline__ AbsDiffRow row(int64_t r) const { return AbsDiffRow{x + r * n, center[r]}; }
};

__device__ __forceinline__ float target(float c, float u, float scale) { return u + (c - u) * scale; }

// |target - mean| of one of the two targets (which: 0 mimic, 1 cfg; means [rows][2])
struct AbsCentredRow {
  const float *c, *u;
  float scale, mean;
  __device__ __forceinline__ float signed_at(int64_t i) const { return target(c[i], u[i], scale) - mean; }
  __device__ __forceinline__ float operator()(int64_t i) const { return fabsf(signed_at(i)); }
};
struct AbsCentred {
  const float *cond, *uncond, *means;
  int n, which;
  float scale;
  __device__ __forceinline__ AbsCentredRow row(int64_t r) const { return AbsCentredRow{cond + r * n, uncond + r * n, scale, means[r * 2 + which]}; }
};

// every value of the group's rows, the workgroup's threads striding over each row
template <class F, class Body>
__device__ __forceinline__ void for_each_value(const F& f, int64_t row0, int nrows, int n, Body body) {
  for (int r = 0; r < nrows; ++r) {
    const auto acc = f.row(row0 + r);
    for (int64_t i = threadIdx.x; i < n; i += SEL_TPB) body(acc(i));
  }
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// the largest bit pattern of the group (= its largest value: non-negative floats order like their bits)
template <class F>
__device__ uint32_t group_max_bits(const F& f, int64_t row0, int nrows, int n, SelShared& s) {
  __syncthreads();
  if (threadIdx.x == 0) s.ext = 0u;
  __syncthreads();
  uint32_t m = 0u;
  for_each_value(f, row0, nrows, n, [&](float v) { m = max(m, __float_as_uint(v)); });
  m = wave_max_u32(m);
  if ((threadIdx.x & 63) == 0) atomicMax(&s.ext, m);
  __syncthreads();
  return s.ext;
}

// the bit patterns of the k-th smallest value of the group (k from 0) and, if `want_next`, of the (k+1)-th; else v_hi = v_lo
template <class F>
__device__ void select_pair(const F& f, int64_t row0, int nrows, int n, uint32_t k, bool want_next, SelShared& s, uint32_t& v_lo, uint32_t& v_hi) {
  uint32_t prefix = 0u, mask = 0u, cnt = 0u;
  constexpr int SHIFT[3] = {20, 9, 0}, NBINS[3] = {2048, 2048, 512};
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = SHIFT[pass], nb = NBINS[pass];
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += SEL_TPB) s.hist[b] = 0u;
    __syncthreads();
    for_each_value(f, row0, nrows, n, [&](float v) {
      const uint32_t bits = __float_as_uint(v);
      if ((bits & mask) == prefix) atomicAdd(&s.hist[(bits >> shift) & (uint32_t)(nb - 1)], 1u);
    });
    __syncthreads();
    if (threadIdx.x < FMX_WAVE) {   // wave 0: the digit whose bin holds rank k
      const int per = nb / FMX_WAVE, base = (int)threadIdx.x * per;
      uint32_t sum = 0u;
      for (int j = 0; j < per; ++j) sum += s.hist[base + j];
      uint32_t incl = sum;
#pragma unroll
      for (int o = 1; o < FMX_WAVE; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if ((int)threadIdx.x >= o) incl += t;
      }
      const uint32_t excl = incl - sum;
      if (k >= excl && k < incl) {
        uint32_t rem = k - excl;
        int d = base;
        uint32_t c = s.hist[d];
        while (rem >= c && d < base + per - 1) {
          rem -= c;
          c = s.hist[++d];
        }
        s.prefix = prefix | ((uint32_t)d << shift);
        s.k = rem;
        s.cnt = c;
      }
    }
    __syncthreads();
    prefix = s.prefix;
    k = s.k;
    cnt = s.cnt;
    mask |= (uint32_t)(nb - 1) << shift;
  }
  v_lo = prefix;
  v_hi = prefix;
  if (want_next && k + 1u >= cnt) {   // the values equal to v_lo end at rank k: the next one is the smallest above
    __syncthreads();
    if (threadIdx.x == 0) s.ext = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t m = 0xFFFFFFFFu;
    for_each_value(f, row0, nrows, n, [&](float v) {
      const uint32_t bits = __float_as_uint(v);
      if (bits > prefix) m = min(m, bits);
    });
    m = wave_min_u32(m);
    if ((threadIdx.x & 63) == 0) atomicMin(&s.ext, m);
    __syncthreads();
    v_hi = s.ext;
  }
}

// where the quantile sits among N sorted values: pos = q * (N - 1) in fp32, as torch.quantile forms it
struct Rank {
  uint32_t k;
  int want_next, is_max;
  float w;
};
Rank rank_of(float q, int64_t N) {
  const float last = (float)(N - 1);
  volatile float pos_v = q * last;   // one fp32 product, whatever the host compiler would rather do
  const float pos = pos_v;
  const float lo = floorf(pos), hi = ceilf(pos);
  Rank r;
  int64_t k = (int64_t)lo;
  r.want_next = hi != lo;
  if (k >= N - 1) {   // (float)(N - 1) may round up past the last index
    k = N - 1;
    r.want_next = 0;
  }
  r.k = (uint32_t)k;
  r.w = r.want_next ? pos - lo : 0.0f;
  r.is_max = (k == N - 1);
  return r;
}

// torch.lerp as the CPU's vector kernel evaluates it (one fused multiply-add on either side of w = 0.5)
__device__ __forceinline__ float lerp_q(float a, float b, float w) {
  const float diff = b - a;
  return w < 0.5f ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);
}

template <class F>
__device__ float group_quantile(const F& f, int64_t row0, int nrows, int n, Rank rk, SelShared& s) {
  if (rk.is_max) return __uint_as_float(group_max_bits(f, row0, nrows, n, s));
  uint32_t lo, hi;
  select_pair(f, row0, nrows, n, rk.k, rk.want_next != 0, s, lo, hi);
  return lerp_q(__uint_as_float(lo), __uint_as_float(hi), rk.w);
}

__global__ __launch_bounds__(SEL_TPB) void row_abs_quantile_kernel(const float* __restrict__ x, const float* __restrict__ center, int n, int rpg,
                                                                   Rank rk, float* __restrict__ out) {
  __shared__ SelShared s;
  const int64_t row0 = (int64_t)blockIdx.x * rpg;
  const float v = group_quantile(AbsDiff{x, center, n}, row0, rpg, n, rk, s);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// ---- the op ---------------------------------------------------------------------------------------------------------------------------------
struct Workspace {
  float *partial, *means, *refs;
};
inline Workspace carve(float* ws, int64_t rows, int64_t nchunks) {
  Workspace w;
  w.partial = ws;
  w.means = ws + rows * nchunks * 2;
  w.refs = w.means + rows * 2;
  return w;
}

// sum over the workgroup, the same on every thread: xor-butterfly inside a wave, the waves added in order.  `red` holds one float per wave.
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) t += red[k];
  return t;
}

// grid (nchunks, rows): the chunk's sums of the two targets (a thread adds its values in index order, then block_sum)
__global__ __launch_bounds__(TPB) void dynthresh_partial_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, int hw, int nchunks,
                                                                float mimic, float cfg, Workspace w) {
  __shared__ float red[2 * (TPB / FMX_WAVE)];
  const int64_t row = blockIdx.y, start = (int64_t)blockIdx.x * CHUNK;
  const int cnt = (int)min((int64_t)CHUNK, hw - start);
  const float* c = cond + row * hw + start;
  const float* u = uncond + row * hw + start;
  float sm = 0.f, sc = 0.f;
  for (int i = threadIdx.x; i < cnt; i += TPB) {
    const float cv = c[i], uv = u[i];
    sm += target(cv, uv, mimic);
    sc += target(cv, uv, cfg);
  }
  sm = block_sum<TPB / FMX_WAVE>(sm, red);
  sc = block_sum<TPB / FMX_WAVE>(sc, red + TPB / FMX_WAVE);
  if (threadIdx.x == 0) {
    float* dst = w.partial + (row * nchunks + blockIdx.x) * 2;
    dst[0] = sm;
    dst[1] = sc;
  }
}

// grid (groups): the means of the group's rows (partials added in chunk order), then the two scale references of the group
__global__ __launch_bounds__(SEL_TPB) void dynthresh_refs_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, int hw, int nchunks,
                                                                 int rpg, float mimic, float cfg, Rank rk, int flags, Workspace w) {
  __shared__ SelShared s;
  const int64_t row0 = (int64_t)blockIdx.x * rpg;
  for (int r = threadIdx.x; r < rpg; r += SEL_TPB) {
    const float* src = w.partial + (row0 + r) * nchunks * 2;
    float sm = 0.f, sc = 0.f;
    for (int k = 0; k < nchunks; ++k) {
      sm += src[2 * (int64_t)k];
      sc += src[2 * (int64_t)k + 1];
    }
    w.means[(row0 + r) * 2] = sm / (float)hw;
    w.means[(row0 + r) * 2 + 1] = sc / (float)hw;
  }
  __syncthreads();   // the means are read back by every thread below
  const AbsCentred fm{cond, uncond, w.means, hw, 0, mimic}, fc{cond, uncond, w.means, hw, 1, cfg};
  float mim_ref, cfg_ref;
  if (flags & FMX_DYNTHRESH_STD) {
    // torch.std of the centred values: their own mean first (rounding-level, not zero), then the squared distances from it, over N - 1
    const float count = (float)((int64_t)rpg * hw);
    float am = 0.f, ac = 0.f;
    for (int r = 0; r < rpg; ++r) {
      const AbsCentredRow a = fm.row(row0 + r), b = fc.row(row0 + r);
      for (int64_t i = threadIdx.x; i < hw; i += SEL_TPB) {
        am += a.signed_at(i);
        ac += b.signed_at(i);
      }
    }
    const float mm = block_sum<SEL_WAVES>(am, s.red) / count, mc = block_sum<SEL_WAVES>(ac, s.red + SEL_WAVES) / count;
    float qm = 0.f, qc = 0.f;
    for (int r = 0; r < rpg; ++r) {
      const AbsCentredRow a = fm.row(row0 + r), b = fc.row(row0 + r);
      for (int64_t i = threadIdx.x; i < hw; i += SEL_TPB) {
        const float dm = a.signed_at(i) - mm, dc = b.signed_at(i) - mc;
        qm += dm * dm;
        qc += dc * dc;
      }
    }
    mim_ref = sqrtf(block_sum<SEL_WAVES>(qm, s.red) / (count - 1.0f));
    cfg_ref = sqrtf(block_sum<SEL_WAVES>(qc, s.red + SEL_WAVES) / (count - 1.0f));
  } else {
    mim_ref = __uint_as_float(group_max_bits(fm, row0, rpg, hw, s));
    cfg_ref = group_quantile(fc, row0, rpg, hw, rk, s);
  }
  if (threadIdx.x == 0) {
    w.refs[blockIdx.x * 2] = mim_ref;
    w.refs[blockIdx.x * 2 + 1] = cfg_ref;
  }
}

// grid (nchunks, rows)
__global__ __launch_bounds__(TPB) void dynthresh_apply_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, int hw, int rpg,
                                                              float mimic, float cfg, int flags, int interpolate, float phi, float one_minus_phi,
                                                              Workspace w, float* __restrict__ out) {
  const int64_t row = blockIdx.y, start = (int64_t)blockIdx.x * CHUNK;
  const int cnt = (int)min((int64_t)CHUNK, hw - start);
  const int64_t group = row / rpg;
  const float mim_ref = w.refs[group * 2], cfg_ref = w.refs[group * 2 + 1], cfg_mean = w.means[row * 2 + 1];
  const float* c = cond + row * hw + start;
  const float* u = uncond + row * hw + start;
  float* o = out + row * hw + start;
  const float factor = mim_ref / cfg_ref, m = fmaxf(mim_ref, cfg_ref);
  for (int i = threadIdx.x; i < cnt; i += TPB) {
    const float t = target(c[i], u[i], cfg);
    float res;
    if (flags & FMX_DYNTHRESH_ZERO) {
      res = t * factor;
    } else {
      const float centred = t - cfg_mean;
      if (flags & FMX_DYNTHRESH_STD)
        res = centred / cfg_ref * mim_ref + cfg_mean;
      else
        res = fminf(fmaxf(centred, -m), m) / m * mim_ref + cfg_mean;
    }
    if (interpolate) res = res * phi + t * one_minus_phi;
    o[i] = res;
  }
}

}  // namespace

extern "C" int fmx_row_abs_quantile_f32(const float* x, const float* center, int32_t rows, int32_t n, int32_t rows_per_group, float q, float* out,
                                        void* stream) {
  FMX_REQUIRE(x && center && out, "row_abs_quantile: null pointer");
  FMX_REQUIRE(rows > 0 && n > 0 && rows_per_group > 0, "row_abs_quantile: bad dims rows=%d n=%d rows_per_group=%d", rows, n, rows_per_group);
  FMX_REQUIRE(rows % rows_per_group == 0, "row_abs_quantile: %d rows are not whole groups of %d", rows, rows_per_group);
  const int64_t N = (int64_t)rows_per_group * n;
  FMX_REQUIRE(N <= 0x7FFFFFFFLL, "row_abs_quantile: a group of %lld values is out of range (2^31 - 1 at most)", (long long)N);
  FMX_REQUIRE(q >= 0.0f && q <= 1.0f, "row_abs_quantile: q must lie in [0, 1], got %g", (double)q);
  hipLaunchKernelGGL(row_abs_quantile_kernel, dim3(rows / rows_per_group), dim3(SEL_TPB), 0, (hipStream_t)stream, x, center, n, rows_per_group,
                     rank_of(q, N), out);
  FMX_LAUNCH_CHECK("fmx_row_abs_quantile_f32");
  return 0;
}

extern "C" int fmx_dynthresh_f32(const float* cond, const float* uncond, int32_t b, int32_t c, int32_t hw, float mimic, float cfg, float percentile,
                                 int32_t flags, double phi, float* workspace, float* out, void* stream) {
  FMX_REQUIRE(cond && uncond && workspace && out, "dynthresh: null pointer");
  FMX_REQUIRE(out != cond && out != uncond, "dynthresh: out may alias neither input");
  FMX_REQUIRE(fmx_aligned16(workspace), "dynthresh: the workspace must be 16-byte aligned");
  FMX_REQUIRE(b > 0 && c > 0 && hw > 0, "dynthresh: bad dims b=%d c=%d hw=%d", b, c, hw);
  const int64_t rows = (int64_t)b * c, total = rows * hw;
  FMX_REQUIRE(rows <= 65535 && total <= 0x7FFFFFFFLL, "dynthresh: %lld rows of %d values are out of range", (long long)rows, hw);
  FMX_REQUIRE(percentile >= 0.0f && percentile <= 1.0f, "dynthresh: the percentile must lie in [0, 1], got %g", (double)percentile);
  FMX_REQUIRE((flags & ~(FMX_DYNTHRESH_SEPARATE | FMX_DYNTHRESH_ZERO | FMX_DYNTHRESH_STD)) == 0, "dynthresh: unknown flag bits in %d", flags);
  const int nchunks = (int)FMX_DYNTHRESH_NCHUNKS(hw);
  const int rpg = (flags & FMX_DYNTHRESH_SEPARATE) ? 1 : (int)rows;
  const Workspace w = carve(workspace, rows, nchunks);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dynthresh_partial_kernel, dim3(nchunks, (unsigned)rows), dim3(TPB), 0, st, cond, uncond, hw, nchunks, mimic, cfg, w);
  FMX_LAUNCH_CHECK("fmx_dynthresh_f32 (partial sums)");
  hipLaunchKernelGGL(dynthresh_refs_kernel, dim3((unsigned)(rows / rpg)), dim3(SEL_TPB), 0, st, cond, uncond, hw, nchunks, rpg, mimic, cfg,
                     rank_of(percentile, (int64_t)rpg * hw), flags, w);
  FMX_LAUNCH_CHECK("fmx_dynthresh_f32 (references)");
  // the reference multiplies by the Python floats phi and 1.0 - phi, each rounded to fp32 once
  hipLaunchKernelGGL(dynthresh_apply_kernel, dim3(nchunks, (unsigned)rows), dim3(TPB), 0, st, cond, uncond, hw, rpg, mimic, cfg, flags,
                     phi != 1.0 ? 1 : 0, (float)phi, (float)(1.0 - phi), w, out);
  FMX_LAUNCH_CHECK("fmx_dynthresh_f32 (apply)");
  return 0;
}
