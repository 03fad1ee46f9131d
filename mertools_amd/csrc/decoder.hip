// decoder.hip — the operators the decoder-only text models need on top of the existing ones (mertools_amd/llama.py, mertools_amd/bloom.py):
//   mer_rmsnorm          HF LlamaRMSNorm: (x * rsqrt(mean(x^2) + eps)) * gamma      -> fp32 and/or 16-bit planes
//   mer_layernorm_row    F.layer_norm for rows up to 8192 wide: (x - mean) * rsqrt(var + eps) * gamma + beta, centred variance
//   mer_rope_attention   causal softmax attention on fp32 q | k | v with the rotary embedding applied as q and k are loaded
//   mer_alibi_attention  the same attention with no rotation and the ALiBi bias slopes[h] * (j - t) added to the score
// All are exact fp32 (plain FMAs, every product and sum spelled out, contraction off) and batch-shape invariant: a row's bits are a
// function of that row (the norms) or of rows 0..t of its own sentence (attention), whatever M, B or the right padding T are.
#include "common.h"

namespace mer {

// One workgroup per row, whatever M is (one variant: nothing to keep bit-identical with): thread i holds float4s i, i + 256, ... of the
// row (D <= 8192: at most 8), sums its squares in four lanes of one accumulator, then wave shuffle tree + a fixed tree over the 4 waves.
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma, float eps, int D,
                                                      float* __restrict__ out32, long long ld32, T* __restrict__ ohi, T* __restrict__ olo, long long ld16) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int tid = threadIdx.x, nv4 = D >> 2;
  const long long row = blockIdx.x;
  const float* xr = x + row * ldx;
  f32x4 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j;
    v[j] = idx < nv4 ? *reinterpret_cast<const f32x4*>(xr + idx * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = fmaf(v[j][e], v[j][e], q[e]);
  const float s = wave_sum((q[0] + q[1]) + (q[2] + q[3]));
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float ms = ((red[0] + red[1]) + (red[2] + red[3])) / (float)D;
  const float rstd = 1.0f / sqrtf(ms + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j;
    if (idx < nv4) {
      f32x4 g = {1.f, 1.f, 1.f, 1.f}, y;
      if (gamma) g = *reinterpret_cast<const f32x4*>(gamma + idx * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (v[j][e] * rstd) * g[e];
      if (out32) *reinterpret_cast<f32x4*>(out32 + row * ld32 + idx * 4) = y;
      if (ohi) {
        typename T16<T>::v4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          T hh, ll;
          split16<T>(y[e], hh, ll);
          h[e] = hh;
          l[e] = ll;
        }
        *reinterpret_cast<typename T16<T>::v4*>(ohi + row * ld16 + idx * 4) = h;
        if (olo) *reinterpret_cast<typename T16<T>::v4*>(olo + row * ld16 + idx * 4) = l;
      }
    }
  }
}

// LayerNorm over a row of up to 8192 columns, built like rmsnorm_kernel: one workgroup per row whatever M is, the row in registers.
// Two passes over the registers: the mean, then the sum of squares of the CENTRED values (a row offset by 1e4 keeps its variance,
// where E[x^2] - E[x]^2 would cancel); both with the same fixed trees (four lanes, wave shuffle, four waves).  gamma / beta NULL: 1 / 0.
template <typename T>
__global__ __launch_bounds__(256) void layernorm_row_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int D, float* __restrict__ out32, long long ld32,
                                                            T* __restrict__ ohi, T* __restrict__ olo, long long ld16) {
#pragma clang fp contract(off)
  __shared__ float red[8];
  const int tid = threadIdx.x, nv4 = D >> 2;
  const long long row = blockIdx.x;
  const float* xr = x + row * ldx;
  f32x4 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j;
    v[j] = idx < nv4 ? *reinterpret_cast<const f32x4*>(xr + idx * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = q[e] + v[j][e];
  const float s = wave_sum((q[0] + q[1]) + (q[2] + q[3]));
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)D;
  q = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool in = tid + 256 * j < nv4;             // a column beyond D stays 0: it must not become -mean
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[j][e] = in ? v[j][e] - mean : 0.f;
      q[e] = fmaf(v[j][e], v[j][e], q[e]);
    }
  }
  const float s2 = wave_sum((q[0] + q[1]) + (q[2] + q[3]));
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = s2;
  __syncthreads();
  const float var = ((red[4] + red[5]) + (red[6] + red[7])) / (float)D;
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = tid + 256 * j;
    if (idx < nv4) {
      f32x4 g = {1.f, 1.f, 1.f, 1.f}, bt = {0.f, 0.f, 0.f, 0.f}, y;
      if (gamma) g = *reinterpret_cast<const f32x4*>(gamma + idx * 4);
      if (beta) bt = *reinterpret_cast<const f32x4*>(beta + idx * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (v[j][e] * rstd) * g[e] + bt[e];
      if (out32) *reinterpret_cast<f32x4*>(out32 + row * ld32 + idx * 4) = y;
      if (ohi) {
        typename T16<T>::v4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          T hh, ll;
          split16<T>(y[e], hh, ll);
          h[e] = hh;
          l[e] = ll;
        }
        *reinterpret_cast<typename T16<T>::v4*>(ohi + row * ld16 + idx * 4) = h;
        if (olo) *reinterpret_cast<typename T16<T>::v4*>(olo + row * ld16 + idx * 4) = l;
      }
    }
  }
}

// Causal attention with rotary q / k (ROT) or with the ALiBi bias (!ROT).  Workgroup = (16 consecutive queries, head, sentence), 256 threads; thread = (query qi = tid / 16,
// slot kj = tid % 16).  Keys are walked in chunks of 32 from key 0 up to the tile's last query: a chunk's K rows are rotated while they
// are copied into LDS (each rotated once per 16 queries), its V rows are copied as they are.  Per chunk, thread (qi, kj) owns the scores
// of keys kj and kj + 16, the 16 threads of a query combine their maxima / sums with a shuffle tree, and the same threads then own output
// columns 4 kj .. 4 kj + 3 (+ 64 for head_dim 128) of the query: online softmax in fp32 (running maximum m, sum l, rescaled accumulator).
// What a row computes depends on its own t and on keys 0..t only: a chunk or a key beyond t contributes exp(-inf) = 0 to the sum and is
// not touched by the P V loop (so that even a non-finite value in a later row cannot leak in), and the rescale factor of a chunk that
// holds no visible key is exp(0) = 1 — the bits do not change with B, with T, or with what the padding rows hold.
// The position treatment is the template parameter: ROT rotates q and k rows as they are loaded (cs / sn = the cos / sin tables);
// !ROT copies them and adds slope * (j - t) to the score of key j (cs = the per-head slopes, float[H]; sn is not read).  That is ALiBi
// in its relative form: 0 on the diagonal, <= 0 below it, a function of j - t only, and a zero slope leaves the score's bits alone.
constexpr int RA_QT = 16, RA_KC = 32;

template <typename T, int HD, bool ROT>
__global__ __launch_bounds__(256) void rope_attention_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                             long long ld, const float* __restrict__ cs, const float* __restrict__ sn,
                                                             T* __restrict__ ohi, T* __restrict__ olo, long long ldo, int Tn, float scale) {
#pragma clang fp contract(off)
  constexpr int HALF = HD / 2, H4 = HD / 8;       // H4: float4s in half a head row
  constexpr int LDK = HD + 4;                       // padded LDS row: the 16 keys a wave reads at once fall on distinct banks
  constexpr int NO = HD / 64;                       // output float4s per thread
  __shared__ f32x4 Qs[RA_QT * LDK / 4];
  __shared__ f32x4 Ks[RA_KC * LDK / 4];
  __shared__ f32x4 Vs[RA_KC * HD / 4];
  __shared__ float Ps[RA_QT][RA_KC];
  const int tid = threadIdx.x, qi = tid >> 4, kj = tid & 15;
  const int q0 = blockIdx.x * RA_QT, h = blockIdx.y, b = blockIdx.z;
  const long long row0 = (long long)b * Tn;
  const int kmax = q0 + RA_QT < Tn ? q0 + RA_QT : Tn;     // keys [0, kmax) are all this tile can see
  const int t = q0 + qi;                                   // this thread's query (rows >= Tn compute on zeros and store nothing)

  // rotate_half convention: out[d] = x[d] cos[d] - x[d + HALF] sin[d], out[d + HALF] = x[d + HALF] cos[d] + x[d] sin[d]; !ROT: a copy
  auto rotate_into = [&](f32x4* dst, const float* src, int pos, int c4) __attribute__((always_inline)) {
#pragma clang fp contract(off)
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + c4 * 4);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(src + HALF + c4 * 4);
    if constexpr (ROT) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (long long)pos * HALF + c4 * 4);
      const f32x4 s = *reinterpret_cast<const f32x4*>(sn + (long long)pos * HALF + c4 * 4);
      f32x4 lo, hi;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo[e] = a[e] * c[e] - bb[e] * s[e];
        hi[e] = bb[e] * c[e] + a[e] * s[e];
      }
      dst[c4] = lo;
      dst[H4 + c4] = hi;
    } else {
      dst[c4] = a;
      dst[H4 + c4] = bb;
    }
  };

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < RA_QT * H4; i += 256) {
    const int r = i / H4, c4 = i % H4;
    if (q0 + r < Tn) {
      rotate_into(Qs + r * (LDK / 4), q + (row0 + q0 + r) * ld + h * HD, q0 + r, c4);
    } else {
      Qs[r * (LDK / 4) + c4] = zero4;
      Qs[r * (LDK / 4) + H4 + c4] = zero4;
    }
  }

  float slope = 0.f;
  if constexpr (!ROT) slope = cs[h];
  float m = -INFINITY, l = 0.f;
  f32x4 acc[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) acc[o] = zero4;

  for (int k0 = 0; k0 < kmax; k0 += RA_KC) {
    __syncthreads();                                 // the previous chunk's P V has read Ks / Vs / Ps (first pass: nothing pending)
    for (int i = tid; i < RA_KC * H4; i += 256) {
      const int r = i / H4, c4 = i % H4;
      if (k0 + r < kmax) {
        rotate_into(Ks + r * (LDK / 4), k + (row0 + k0 + r) * ld + h * HD, k0 + r, c4);
        const float* vr = v + (row0 + k0 + r) * ld + h * HD;
        Vs[r * (HD / 4) + c4] = *reinterpret_cast<const f32x4*>(vr + c4 * 4);
        Vs[r * (HD / 4) + H4 + c4] = *reinterpret_cast<const f32x4*>(vr + HALF + c4 * 4);
      } else {
        Ks[r * (LDK / 4) + c4] = zero4;
        Ks[r * (LDK / 4) + H4 + c4] = zero4;
        Vs[r * (HD / 4) + c4] = zero4;
        Vs[r * (HD / 4) + H4 + c4] = zero4;
      }
    }
    __syncthreads();
    // scores of keys k0 + kj and k0 + kj + 16 against query t: four partial sums per key (one per float4 lane), combined pairwise
    f32x4 sa = zero4, sb = zero4;
#pragma unroll 8
    for (int d4 = 0; d4 < HD / 4; ++d4) {
      const f32x4 qv = Qs[qi * (LDK / 4) + d4];
      const f32x4 ka = Ks[kj * (LDK / 4) + d4];
      const f32x4 kb = Ks[(kj + 16) * (LDK / 4) + d4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sa[e] = fmaf(qv[e], ka[e], sa[e]);
        sb[e] = fmaf(qv[e], kb[e], sb[e]);
      }
    }
    float s0 = ((sa[0] + sa[1]) + (sa[2] + sa[3])) * scale;
    float s1 = ((sb[0] + sb[1]) + (sb[2] + sb[3])) * scale;
    if constexpr (!ROT) {                            // j - t is an integer of at most 12 bits: exact in fp32
      s0 = s0 + slope * (float)(k0 + kj - t);
      s1 = s1 + slope * (float)(k0 + kj + 16 - t);
    }
    if (k0 + kj > t) s0 = -INFINITY;                 // a select, not arithmetic: whatever a hidden key holds never enters
    if (k0 + kj + 16 > t) s1 = -INFINITY;
    float cm = fmaxf(s0, s1);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o));
    const float mn = fmaxf(m, cm);                   // finite from the first chunk on: key 0 is visible to every query
    const float alpha = expf(m - mn);                // first chunk: exp(-inf) = 0 on l = 0 and acc = 0
    const float p0 = expf(s0 - mn), p1 = expf(s1 - mn);
    float ps = p0 + p1;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ps += __shfl_xor(ps, o);
    l = l * alpha + ps;
    m = mn;
    Ps[qi][kj] = p0;
    Ps[qi][kj + 16] = p1;
    __syncthreads();
    int kend = t - k0 + 1;                           // keys of this chunk the query sees
    kend = kend > RA_KC ? RA_KC : kend;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[o][e] = acc[o][e] * alpha;
    for (int j = 0; j < kend; ++j) {
      const float p = Ps[qi][j];
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const f32x4 vv = Vs[j * (HD / 4) + o * 16 + kj];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[o][e] = fmaf(p, vv[e], acc[o][e]);
      }
    }
  }
  if (t < Tn) {
    const float inv = 1.0f / l;
    const long long orow = (row0 + t) * ldo + h * HD;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      typename T16<T>::v4 hh4, ll4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float y = acc[o][e] * inv;
        T hh, ll;
        split16<T>(y, hh, ll);
        hh4[e] = hh;
        ll4[e] = ll;
      }
      *reinterpret_cast<typename T16<T>::v4*>(ohi + orow + o * 64 + kj * 4) = hh4;
      if (olo) *reinterpret_cast<typename T16<T>::v4*>(olo + orow + o * 64 + kj * 4) = ll4;
    }
  }
}

}  // namespace mer

extern "C" int mer_rmsnorm(const float* x, long long ldx, const float* gamma, float eps, int M, int D, float* out32, long long ld32,
                           void* out16_hi, void* out16_lo, long long ld16, int dtype, mer_stream_t stream) {
  using namespace mer;
  MER_REQUIRE(x && M > 0, MER_EINVAL, "mer_rmsnorm: bad argument (x NULL or M=%d <= 0)", M);
  MER_REQUIRE(D >= 4 && D <= 8192 && D % 4 == 0, MER_ESHAPE, "mer_rmsnorm: D=%d must be a multiple of 4 in [4, 8192]", D);
  MER_REQUIRE(out32 || out16_hi, MER_EINVAL, "mer_rmsnorm: no output (out32 and out16_hi are both NULL)");
  MER_REQUIRE(!out16_lo || out16_hi, MER_EINVAL, "mer_rmsnorm: out16_lo without out16_hi");
  MER_REQUIRE(dtype == MER_DT_F16 || dtype == MER_DT_BF16, MER_EINVAL, "mer_rmsnorm: bad dtype %d", dtype);
  MER_REQUIRE(ldx >= D && ldx % 4 == 0 && (!out32 || (ld32 >= D && ld32 % 4 == 0)) && (!out16_hi || (ld16 >= D && ld16 % 4 == 0)), MER_ESHAPE,
              "mer_rmsnorm: ldx / ld32 / ld16 must be multiples of 4 and >= D");
  MER_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)out32) & 15) == 0 && (((uintptr_t)out16_hi | (uintptr_t)out16_lo) & 7) == 0, MER_ESHAPE,
              "mer_rmsnorm: x, gamma and out32 must be 16-byte aligned, the 16-bit planes 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("rmsnorm", 0.0, (double)M * D * (4 + (out32 ? 4 : 0) + (out16_hi ? 2 : 0) + (out16_lo ? 2 : 0)), st);
  if (dtype == MER_DT_F16)
    hipLaunchKernelGGL((rmsnorm_kernel<f16>), dim3((unsigned)M), dim3(256), 0, st, x, ldx, gamma, eps, D, out32, ld32, (f16*)out16_hi, (f16*)out16_lo, ld16);
  else
    hipLaunchKernelGGL((rmsnorm_kernel<bf16>), dim3((unsigned)M), dim3(256), 0, st, x, ldx, gamma, eps, D, out32, ld32, (bf16*)out16_hi, (bf16*)out16_lo, ld16);
  return check_launch("rmsnorm");
}

extern "C" int mer_rope_attention(const float* q, const float* k, const float* v, long long ld, const float* cos, const float* sin,
                                  void* out_hi, void* out_lo, long long ldo, int B, int T, int H, int head_dim, float scale, int dtype,
                                  mer_stream_t stream) {
  using namespace mer;
  MER_REQUIRE(q && k && v && cos && sin && out_hi, MER_EINVAL, "mer_rope_attention: NULL pointer (q, k, v, cos, sin and out_hi are required)");
  MER_REQUIRE(head_dim == 64 || head_dim == 128, MER_EUNSUPPORTED, "mer_rope_attention: head_dim=%d (64 or 128 only)", head_dim);
  MER_REQUIRE(T >= 1 && T <= 2048, MER_EUNSUPPORTED, "mer_rope_attention: T=%d outside [1, 2048]", T);
  MER_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535, MER_EINVAL, "mer_rope_attention: B=%d, H=%d outside [1, 65535]", B, H);
  MER_REQUIRE(dtype == MER_DT_F16 || dtype == MER_DT_BF16, MER_EINVAL, "mer_rope_attention: bad dtype %d", dtype);
  MER_REQUIRE(ld % 4 == 0 && ld >= (long long)H * head_dim && ldo % 4 == 0 && ldo >= (long long)H * head_dim, MER_ESHAPE,
              "mer_rope_attention: ld and ldo must be multiples of 4 and >= H * head_dim");
  MER_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)cos | (uintptr_t)sin) & 15) == 0 && (((uintptr_t)out_hi | (uintptr_t)out_lo) & 7) == 0,
              MER_ESHAPE, "mer_rope_attention: q, k, v, cos and sin must be 16-byte aligned, the output planes 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(T, RA_QT), (unsigned)H, (unsigned)B), block(256);
  // causal: half of the T x T score matrix, twice (q k^T and p v)
  ProfScope prof("rope_attention", 2.0 * B * H * (double)T * T * head_dim, (double)B * T * H * head_dim * (12 + 2 + (out_lo ? 2 : 0)), st);
#define MER_RA_LAUNCH(TT, HDV) \
  hipLaunchKernelGGL((rope_attention_kernel<TT, HDV, true>), grid, block, 0, st, q, k, v, ld, cos, sin, (TT*)out_hi, (TT*)out_lo, ldo, T, scale)
  if (dtype == MER_DT_F16) {
    if (head_dim == 64) MER_RA_LAUNCH(f16, 64);
    else MER_RA_LAUNCH(f16, 128);
  } else {
    if (head_dim == 64) MER_RA_LAUNCH(bf16, 64);
    else MER_RA_LAUNCH(bf16, 128);
  }
#undef MER_RA_LAUNCH
  return check_launch("rope_attention");
}

extern "C" int mer_layernorm_row(const float* x, long long ldx, const float* gamma, const float* beta, float eps, int M, int D, float* out32,
                                 long long ld32, void* out16_hi, void* out16_lo, long long ld16, int dtype, mer_stream_t stream) {
  using namespace mer;
  MER_REQUIRE(x && M > 0, MER_EINVAL, "mer_layernorm_row: bad argument (x NULL or M=%d <= 0)", M);
  MER_REQUIRE(D >= 4 && D <= 8192 && D % 4 == 0, MER_ESHAPE, "mer_layernorm_row: D=%d must be a multiple of 4 in [4, 8192]", D);
  MER_REQUIRE(out32 || out16_hi, MER_EINVAL, "mer_layernorm_row: no output (out32 and out16_hi are both NULL)");
  MER_REQUIRE(!out16_lo || out16_hi, MER_EINVAL, "mer_layernorm_row: out16_lo without out16_hi");
  MER_REQUIRE(dtype == MER_DT_F16 || dtype == MER_DT_BF16, MER_EINVAL, "mer_layernorm_row: bad dtype %d", dtype);
  MER_REQUIRE(ldx >= D && ldx % 4 == 0 && (!out32 || (ld32 >= D && ld32 % 4 == 0)) && (!out16_hi || (ld16 >= D && ld16 % 4 == 0)), MER_ESHAPE,
              "mer_layernorm_row: ldx / ld32 / ld16 must be multiples of 4 and >= D");
  MER_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out32) & 15) == 0 && (((uintptr_t)out16_hi | (uintptr_t)out16_lo) & 7) == 0,
              MER_ESHAPE, "mer_layernorm_row: x, gamma, beta and out32 must be 16-byte aligned, the 16-bit planes 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("layernorm_row", 0.0, (double)M * D * (4 + (out32 ? 4 : 0) + (out16_hi ? 2 : 0) + (out16_lo ? 2 : 0)), st);
  if (dtype == MER_DT_F16)
    hipLaunchKernelGGL((layernorm_row_kernel<f16>), dim3((unsigned)M), dim3(256), 0, st, x, ldx, gamma, beta, eps, D, out32, ld32, (f16*)out16_hi,
                       (f16*)out16_lo, ld16);
  else
    hipLaunchKernelGGL((layernorm_row_kernel<bf16>), dim3((unsigned)M), dim3(256), 0, st, x, ldx, gamma, beta, eps, D, out32, ld32, (bf16*)out16_hi,
                       (bf16*)out16_lo, ld16);
  return check_launch("layernorm_row");
}

extern "C" int mer_alibi_attention(const float* q, const float* k, const float* v, long long ld, const float* slopes, void* out_hi, void* out_lo,
                                   long long ldo, int B, int T, int H, int head_dim, float scale, int dtype, mer_stream_t stream) {
  using namespace mer;
  MER_REQUIRE(q && k && v && slopes && out_hi, MER_EINVAL, "mer_alibi_attention: NULL pointer (q, k, v, slopes and out_hi are required)");
  MER_REQUIRE(head_dim == 64 || head_dim == 128, MER_EUNSUPPORTED, "mer_alibi_attention: head_dim=%d (64 or 128 only)", head_dim);
  MER_REQUIRE(T >= 1 && T <= 2048, MER_EUNSUPPORTED, "mer_alibi_attention: T=%d outside [1, 2048]", T);
  MER_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535, MER_EINVAL, "mer_alibi_attention: B=%d, H=%d outside [1, 65535]", B, H);
  MER_REQUIRE(dtype == MER_DT_F16 || dtype == MER_DT_BF16, MER_EINVAL, "mer_alibi_attention: bad dtype %d", dtype);
  MER_REQUIRE(ld % 4 == 0 && ld >= (long long)H * head_dim && ldo % 4 == 0 && ldo >= (long long)H * head_dim, MER_ESHAPE,
              "mer_alibi_attention: ld and ldo must be multiples of 4 and >= H * head_dim");
  MER_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0 && ((uintptr_t)slopes & 3) == 0 && (((uintptr_t)out_hi | (uintptr_t)out_lo) & 7) == 0,
              MER_ESHAPE, "mer_alibi_attention: q, k and v must be 16-byte aligned, slopes 4-byte, the output planes 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(T, RA_QT), (unsigned)H, (unsigned)B), block(256);
  ProfScope prof("alibi_attention", 2.0 * B * H * (double)T * T * head_dim, (double)B * T * H * head_dim * (12 + 2 + (out_lo ? 2 : 0)), st);
#define MER_AA_LAUNCH(TT, HDV) \
  hipLaunchKernelGGL((rope_attention_kernel<TT, HDV, false>), grid, block, 0, st, q, k, v, ld, slopes, (const float*)nullptr, (TT*)out_hi, (TT*)out_lo, ldo, T, scale)
  if (dtype == MER_DT_F16) {
    if (head_dim == 64) MER_AA_LAUNCH(f16, 64);
    else MER_AA_LAUNCH(f16, 128);
  } else {
    if (head_dim == 64) MER_AA_LAUNCH(bf16, 64);
    else MER_AA_LAUNCH(bf16, 128);
  }
#undef MER_AA_LAUNCH
  return check_launch("alibi_attention");
}
