// model.hip — correction-model forward on gfx950 (replaces the libtorch call at reference
// src/inference.rs:152-172).  See model_dev.h for the (assumed) architecture.
//
// Exactness note: the conv stack and the per-position linear are evaluated ONLY for the rows the
// reference's model gathers (`indices`, inference.rs:136-141), over the receptive field of each
// such row.  A dense evaluation over all L x 31 cells followed by the gather gives the same
// numbers, 30-100x slower; the batch-padding cells the dense model would see near a window's tail
// (token 11 / quality 126 up to the batch's max length, zeros beyond — inference.rs:86-97) are
// reproduced exactly.
//
// GEMMs run on the matrix cores.  precision 0: v_mfma_f32_16x16x4_f32 (exact f32);
// precision 1: v_mfma_f32_16x16x32_bf16 on a hi/lo bf16 split of both operands, 3 MFMAs per
// k-step (a*b ~= ah*bh + ah*bl + al*bh, ~2^-16 relative) — this is what keeps logits inside the
// 1e-3 contract while running ~5x the f32 MFMA rate; precision 2: plain VALU (debug reference).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "model_dev.h"

namespace herro {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

// inference.rs:16-21,153: x = QUAL_SCALE * q - QUAL_OFFSET in f32 — as ONE fused multiply-add, spelled out.  The reference rounds twice (a product, then a
// difference); this function used to say so with __fmul_rn / __fsub_rn, but those are a plain `*` and `-` in the HIP headers, and the compiler contracted them into
// one v_fmac wherever the argument is a run-time value (127 of the 256 byte values one ulp away from the two-rounding result: 126 -> 0.99999994, not 1.0) while it
// folded a constant argument with two roundings.  So a batch-padding cell that the job's front end supplies by addressing (norm_qual(126u) below) and the same cell
// read from a caller's dense planes (herro_model_forward) differed in the last bit (tests/test_gpu_rf_models.py).  The fused form is what every kernel has computed
// on real cells all along, and what the load-time calibration figures were measured with; writing it explicitly makes constants and run-time values agree and
// takes the result out of the compiler's contraction setting.  (Against the reference's two roundings that is at most 6e-8 on an input in [-1, 1].)
__device__ __forceinline__ float norm_qual(uint32_t q) {
  const float QS = (float)(2.0 / 93.0);
  const float QO = (float)(2.0 * 33.0 / 93.0 + 1.0);
  return __builtin_fmaf(QS, (float)q, -QO);
}

// gfx950 converts f32 -> bf16 (round to nearest even) in hardware: v_cvt_pk_bf16_f32, one instruction per
// PAIR of values; the integer sequence it replaces was ~5 VALU ops per value and made the split epilogues
// (and conv1's on-the-fly A tile) VALU-bound.
typedef __bf16 hbf16x2 __attribute__((ext_vector_type(2)));
typedef float hf32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
// (a, b) -> packed bf16 pairs hi, lo with a ~= hi.x + lo.x, b ~= hi.y + lo.y (5 instructions)
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  const hf32x2 v = {a, b};
  hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hbf16x2));
  const hf32x2 hf = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(v - hf, hbf16x2));
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// ---------------------------------------------------------------------------------------------------
// token table
// ---------------------------------------------------------------------------------------------------
__global__ void k_build_tokens(BatchDev B, ModelScratch S) {
  const uint32_t b = blockIdx.x;
  const uint32_t t0 = B.tok_off[b], t1 = B.tok_off[b + 1];
  for (uint32_t n = t0 + threadIdx.x; n < t1; n += blockDim.x) {
    const uint32_t row = B.sup_row[B.sup_off[b] + (n - t0)];
    S.tok_win[n] = b;
    S.tok_row[n] = row;
    S.tok_out[n] = B.out_off[b] + (n - t0);   // (read by k_layers_p when the f16 stack runs behind this front end)
    TokMeta tm;
    tm.plane_off = B.plane_off[b];
    tm.plane_ld = B.plane_ld[b];
    tm.tok_row = row;
    tm.len = B.len[b];
    tm.lmax = B.lmax[b];
    tm.rf_idx = (uint32_t)((B.rf_base ? B.rf_base[b] : B.out_off[b]) + (n - t0));
    tm.pad1 = 0;
    S.tok_meta[n] = tm;
  }
}

// ---------------------------------------------------------------------------------------------------
// embedding + quality channel + conv1 (+BN folded) + ReLU on the receptive field of one token.
// One workgroup per token.  y1[n][r][dl][c] = conv1 output of read row r at position l+dl-h.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_patch_conv1(ModelDev M, BatchDev B, ModelScratch S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t kw = M.h.kw, c1 = M.h.c1, h = kw / 2, P = 4 * h + 1;
  float* s_t1 = reinterpret_cast<float*>(smem);  // [kw][12][c1]
  float* s_wq = s_t1 + kw * 12 * c1;              // [kw][c1]
  float* s_b1 = s_wq + kw * c1;                   // [c1]
  float* s_qn = s_b1 + c1;                        // [31][P] normalised quality (0 where invalid)
  uint32_t* s_tok = reinterpret_cast<uint32_t*>(s_qn + HERRO_ROWS * P);  // [31][P] token, 255 = outside

  const uint32_t n = blockIdx.x;
  const uint32_t b = S.tok_win[n];
  const int32_t l = (int32_t)S.tok_row[n];
  const int32_t len = (int32_t)B.len[b], lmax = (int32_t)B.lmax[b];
  const uint8_t* pb = B.planes_b + B.plane_off[b];
  const uint8_t* pq = B.planes_q + B.plane_off[b];
  const uint32_t ld = B.plane_ld[b];
  const uint8_t* rq = (B.rf_q && P <= 8) ? B.rf_q + ((B.rf_base ? B.rf_base[b] : B.out_off[b]) + (n - B.tok_off[b])) * HERRO_ROWS * 16 : nullptr;   // the token's receptive fields, compact: per read row 8 tokens + 8 qualities (k_rfq)

  for (uint32_t e = threadIdx.x; e < kw * 12 * c1; e += blockDim.x) s_t1[e] = M.t1[e];
  for (uint32_t e = threadIdx.x; e < kw * c1; e += blockDim.x) s_wq[e] = M.wq1[e];
  for (uint32_t e = threadIdx.x; e < c1; e += blockDim.x) s_b1[e] = M.b1[e];
  for (uint32_t e = threadIdx.x; e < HERRO_ROWS * P; e += blockDim.x) {
    const uint32_t r = e / P;
    const int32_t q = l - 2 * (int32_t)h + (int32_t)(e % P);
    uint32_t tok = 255u;
    float qn = 0.f;
    if (q >= 0 && q < lmax) {
      if (q < len) {
        tok = rq ? rq[r * 16 + e % P] : pb[(uint64_t)r * ld + q];
        qn = norm_qual(rq ? rq[r * 16 + 8 + e % P] : pq[(uint64_t)r * ld + q]);
      } else {  // batch padding (inference.rs:86-97)
        tok = TOK_PAD;
        qn = norm_qual(126u);
      }
    }
    s_tok[e] = tok;
    s_qn[e] = qn;
  }
  __syncthreads();

  float* y1 = S.y1 + (uint64_t)n * HERRO_ROWS * kw * c1;
  const uint32_t total = HERRO_ROWS * kw * c1;
  for (uint32_t e = threadIdx.x; e < total; e += blockDim.x) {
    const uint32_t c = e % c1, dl = (e / c1) % kw, r = e / (c1 * kw);
    const int32_t pos = l + (int32_t)dl - (int32_t)h;
    float v = 0.f;
    if (pos >= 0 && pos < lmax) {  // outside: conv2's zero padding
      v = s_b1[c];
      for (uint32_t t = 0; t < kw; t++) {
        const uint32_t pi = dl + t;  // patch index of position pos + t - h
        const uint32_t tok = s_tok[r * P + pi];
        if (tok != 255u) v += s_t1[(t * 12 + tok) * c1 + c] + s_wq[t * c1 + c] * s_qn[r * P + pi];
      }
      v = fmaxf(v, 0.f);
    }
    y1[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------------
// Generic GEMM: C[M,N] = epi(A[M,K] . W[K,N] + bias) (+ R).  W is stored transposed ([N][K]).
// 64x64 tile per workgroup (4 waves as 2x2, each 32x32 = 2x2 MFMA 16x16 tiles), BK = 32.
// ---------------------------------------------------------------------------------------------------
// activation codes of the GEMM epilogues (the `relu` argument of rounds 1-5, widened in round 6): 0 none, 1 ReLU, 2 GELU (erf), 3 GELU (tanh approximation) —
// torch.nn.functional.gelu's two forms, for archives whose encoder was built with activation = "gelu"
__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
  if (act == 3) return 0.5f * v * (1.0f + tanhf(0.79788456080286535588f * (v + 0.044715f * v * v * v)));
  return v;
}
static constexpr int BM = 64, BN = 64, BK = 32;
static constexpr int LDH = BK + 8;  // bf16 row stride (80 B: keeps 16-B alignment, spreads banks)
static constexpr int LDF = BK + 1;  // f32 row stride

template <int MODE>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ A, uint32_t lda, Weight W,
                                              float* C, uint32_t ldc, const float* R, uint32_t M,
                                              int relu) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[(MODE == 1) ? 4 * BM * LDH * 2 : 2 * BM * LDF * 4];
  const uint32_t K = W.K, N = W.N;
  const uint32_t m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t wy = wave >> 1, wx = wave & 1;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float vacc[4][4];  // MODE 2
  if (MODE == 2) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) vacc[i][j] = 0.f;
  }

  for (uint32_t k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    if constexpr (MODE == 1) {
      uint16_t* a_hi = reinterpret_cast<uint16_t*>(smem);
      uint16_t* a_lo = a_hi + BM * LDH;
      uint16_t* b_hi = a_lo + BM * LDH;
      uint16_t* b_lo = b_hi + BN * LDH;
      // A: 64x32 f32 -> split on the fly
#pragma unroll
      for (int it = 0; it < 2; it++) {
        const uint32_t e = tid + it * 256, row = e >> 3, c4 = (e & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m0 + row < M) v = *reinterpret_cast<const float4*>(A + (uint64_t)(m0 + row) * lda + k0 + c4);
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint16_t hb = f32_to_bf16_rne(f[q]);
          a_hi[row * LDH + c4 + q] = hb;
          a_lo[row * LDH + c4 + q] = f32_to_bf16_rne(f[q] - bf16_to_f32(hb));
        }
      }
      {  // W^T hi/lo: 64 rows x 32 bf16 = 4 x 16 B per row
        const uint32_t row = tid >> 2, c8 = (tid & 3) * 8;
        uint4 vh = make_uint4(0, 0, 0, 0), vl = make_uint4(0, 0, 0, 0);
        if (n0 + row < N) {
          vh = *reinterpret_cast<const uint4*>(W.hi + (uint64_t)(n0 + row) * K + k0 + c8);
          vl = *reinterpret_cast<const uint4*>(W.lo + (uint64_t)(n0 + row) * K + k0 + c8);
        }
        *reinterpret_cast<uint4*>(b_hi + row * LDH + c8) = vh;
        *reinterpret_cast<uint4*>(b_lo + row * LDH + c8) = vl;
      }
      __syncthreads();
      const uint32_t fr = lane & 15, fk = (lane >> 4) * 8;
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        ah[i] = *reinterpret_cast<const bf16x8*>(a_hi + (wy * 32 + i * 16 + fr) * LDH + fk);
        al[i] = *reinterpret_cast<const bf16x8*>(a_lo + (wy * 32 + i * 16 + fr) * LDH + fk);
        bh[i] = *reinterpret_cast<const bf16x8*>(b_hi + (wx * 32 + i * 16 + fr) * LDH + fk);
        bl[i] = *reinterpret_cast<const bf16x8*>(b_lo + (wx * 32 + i * 16 + fr) * LDH + fk);
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    } else {
      float* as = reinterpret_cast<float*>(smem);
      float* bs = as + BM * LDF;
#pragma unroll
      for (int it = 0; it < 2; it++) {
        const uint32_t e = tid + it * 256, row = e >> 3, c4 = (e & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m0 + row < M) v = *reinterpret_cast<const float4*>(A + (uint64_t)(m0 + row) * lda + k0 + c4);
        if (n0 + row < N) w = *reinterpret_cast<const float4*>(W.f32 + (uint64_t)(n0 + row) * K + k0 + c4);
        as[row * LDF + c4 + 0] = v.x; as[row * LDF + c4 + 1] = v.y;
        as[row * LDF + c4 + 2] = v.z; as[row * LDF + c4 + 3] = v.w;
        bs[row * LDF + c4 + 0] = w.x; bs[row * LDF + c4 + 1] = w.y;
        bs[row * LDF + c4 + 2] = w.z; bs[row * LDF + c4 + 3] = w.w;
      }
      __syncthreads();
      if constexpr (MODE == 0) {
        const uint32_t fr = lane & 15, fk = lane >> 4;
#pragma unroll
        for (int kk = 0; kk < BK / 4; kk++) {
          float a[2], b[2];
#pragma unroll
          for (int i = 0; i < 2; i++) {
            a[i] = as[(wy * 32 + i * 16 + fr) * LDF + kk * 4 + fk];
            b[i] = bs[(wx * 32 + i * 16 + fr) * LDF + kk * 4 + fk];
          }
#pragma unroll
          for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
      } else {  // MODE 2: VALU, thread owns rows ty*4.., cols tx*4..
        const uint32_t ty = tid >> 4, tx = tid & 15;
        for (int kk = 0; kk < BK; kk++) {
          float a[4], b[4];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            a[i] = as[(ty * 4 + i) * LDF + kk];
            b[i] = bs[(tx * 4 + i) * LDF + kk];
          }
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) vacc[i][j] = fmaf(a[i], b[j], vacc[i][j]);
        }
      }
    }
  }

  // ---- epilogue
  if constexpr (MODE == 2) {
    const uint32_t ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
        if (m < M && n < N) {
          float v = vacc[i][j] + (W.bias ? W.bias[n] : 0.f);
          v = apply_act(v, relu);
          if (R) v += R[(uint64_t)m * ldc + n];
          C[(uint64_t)m * ldc + n] = v;
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const uint32_t n = n0 + wx * 32 + j * 16 + (lane & 15);
        const float bias = (W.bias && n < N) ? W.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t m = m0 + wy * 32 + i * 16 + (lane >> 4) * 4 + r;
          if (m < M && n < N) {
            float v = acc[i][j][r] + bias;
            v = apply_act(v, relu);
            if (R) v += R[(uint64_t)m * ldc + n];
            C[(uint64_t)m * ldc + n] = v;
          }
        }
      }
  }
}

static void gemm(const float* A, uint32_t lda, const Weight& W, float* C, uint32_t ldc, const float* R,
                 uint32_t M, int relu, int precision, hipStream_t st) {
  if (M == 0) return;
  dim3 grid((W.N + BN - 1) / BN, (M + BM - 1) / BM);
  if (precision == 0) hipLaunchKernelGGL(k_gemm<0>, grid, dim3(256), 0, st, A, lda, W, C, ldc, R, M, relu);
  else if (precision == 1) hipLaunchKernelGGL(k_gemm<1>, grid, dim3(256), 0, st, A, lda, W, C, ldc, R, M, relu);
  else hipLaunchKernelGGL(k_gemm<2>, grid, dim3(256), 0, st, A, lda, W, C, ldc, R, M, relu);
}

// ---------------------------------------------------------------------------------------------------
// positional encoding (sinusoidal over the row index), LayerNorm, attention, output scatter
// ---------------------------------------------------------------------------------------------------
__global__ void k_add_pe(ModelDev M, ModelScratch S, uint32_t n_tok) {
  const uint32_t half = M.h.d_model / 2;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_tok * half) return;
  const uint32_t n = (uint32_t)(i / half), k = (uint32_t)(i % half);
  float* x = S.x + (uint64_t)n * M.h.d_model;
  if (M.pe_kind == 1) {   // a learned table, indexed by the row (herro_job_infer / herro_model_forward refuse rows beyond it: the archive would raise there)
    const float2 t = *reinterpret_cast<const float2*>(M.pe_learned + (uint64_t)min(S.tok_row[n], M.pe_learned_rows - 1u) * M.h.d_model + 2 * k);
    x[2 * k] += t.x;
    x[2 * k + 1] += t.y;
    return;
  }
  const float ang = __fmul_rn((float)S.tok_row[n], M.pe_div[k]);
  x[2 * k] += sinf(ang);
  x[2 * k + 1] += cosf(ang);
}

// one wave per row
// (y may be x: Post-LN layers normalise the residual stream in place)
__global__ __launch_bounds__(256) void k_layernorm(const float* x, float* y, const float* g, const float* b,
                                                   uint32_t n_rows, uint32_t D, float eps) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const float* xr = x + (uint64_t)row * D;
  float s = 0.f;
  for (uint32_t i = lane; i < D; i += 64) s += xr[i];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  const float mean = s / (float)D;
  float v = 0.f;
  for (uint32_t i = lane; i < D; i += 64) {
    const float t = xr[i] - mean;
    v += t * t;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  const float rstd = 1.0f / sqrtf(v / (float)D + eps);
  float* yr = y + (uint64_t)row * D;
  for (uint32_t i = lane; i < D; i += 64) yr[i] = (xr[i] - mean) * rstd * g[i] + b[i];
}

// Attention inside one window (its informative positions are the sequence).  One wave per
// (window, head); a lane owns one query row at a time; keys/values are wave-uniform (broadcast)
// loads; online softmax in registers.  head_dim <= 64.
template <int DH>
__global__ __launch_bounds__(64) void k_attention(BatchDev B, ModelScratch S, uint32_t D) {
  const uint32_t b = blockIdx.x, hd = blockIdx.y;
  const uint32_t t0 = B.tok_off[b], len = B.tok_off[b + 1] - t0;
  const float scale = 1.0f / sqrtf((float)DH);
  for (uint32_t i = threadIdx.x; i < len; i += 64) {
    const float* q = S.qkv + (uint64_t)(t0 + i) * 3 * D + hd * DH;
    float qr[DH], o[DH];
#pragma unroll
    for (int d = 0; d < DH; d++) {
      qr[d] = q[d] * scale;
      o[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (uint32_t j = 0; j < len; j++) {
      const float* k = S.qkv + (uint64_t)(t0 + j) * 3 * D + D + hd * DH;
      const float* v = k + D;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DH; d++) s = fmaf(qr[d], k[d], s);
      const float mn = fmaxf(m, s);
      const float alpha = expf(m - mn), p = expf(s - mn);
      l = l * alpha + p;
#pragma unroll
      for (int d = 0; d < DH; d++) o[d] = o[d] * alpha + p * v[d];
      m = mn;
    }
    float* out = S.att + (uint64_t)(t0 + i) * D + hd * DH;
    const float inv = 1.0f / l;
#pragma unroll
    for (int d = 0; d < DH; d++) out[d] = o[d] * inv;
  }
}

__global__ void k_scatter_logits(BatchDev B, ModelScratch S) {
  const uint32_t b = blockIdx.x;
  const uint32_t t0 = B.tok_off[b], t1 = B.tok_off[b + 1];
  for (uint32_t n = t0 + threadIdx.x; n < t1; n += blockDim.x) {
    const float* lg = S.logits + (uint64_t)n * 16;
    const uint64_t o = B.out_off[b] + (n - t0);
    B.out_info[o] = lg[0];
#pragma unroll
    for (int c = 0; c < 5; c++) B.out_base[o * 5 + c] = lg[1 + c];
  }
}

__global__ void k_transpose_blr(const uint8_t* src, uint8_t* dst, uint32_t L) {
  // src [B][L][31] -> dst [B][31][L]
  const uint32_t b = blockIdx.y;
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint8_t* s = src + ((uint64_t)b * L + l) * HERRO_ROWS;
  uint8_t* d = dst + (uint64_t)b * HERRO_ROWS * L + l;
#pragma unroll
  for (int r = 0; r < HERRO_ROWS; r++) d[(uint64_t)r * L] = s[r];
}

void launch_transpose_blr(const uint8_t* src, uint8_t* dst, uint32_t B, uint32_t L, hipStream_t st) {
  hipLaunchKernelGGL(k_transpose_blr, dim3((L + 255) / 256, B), dim3(256), 0, st, src, dst, L);
}


// ===================================================================================================
// bf16x3 pipeline (precision 1)
// ===================================================================================================
__device__ __forceinline__ void split_store(uint16_t* hi, uint16_t* lo, uint64_t idx, float v) {
  const uint16_t h = f32_to_bf16_rne(v);
  hi[idx] = h;
  lo[idx] = f32_to_bf16_rne(v - bf16_to_f32(h));
}

// conv1 on the receptive fields of TOKB tokens per workgroup (tables loaded once), output pre-split.
static constexpr int TOKB = 8;
__global__ __launch_bounds__(256) void k_patch_conv1_s(ModelDev M, BatchDev B, ModelScratch S, uint32_t n_tok) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t kw = M.h.kw, c1 = M.h.c1, h = kw / 2, P = 4 * h + 1;
  float* s_t1 = reinterpret_cast<float*>(smem);  // [kw][12][c1]
  float* s_wq = s_t1 + kw * 12 * c1;              // [kw][c1]
  float* s_b1 = s_wq + kw * c1;                   // [c1]
  float* s_qn = s_b1 + c1;                        // [31][P]
  uint32_t* s_tok = reinterpret_cast<uint32_t*>(s_qn + HERRO_ROWS * P);  // [31][P], 255 = outside
  for (uint32_t e = threadIdx.x; e < kw * 12 * c1; e += blockDim.x) s_t1[e] = M.t1[e];
  for (uint32_t e = threadIdx.x; e < kw * c1; e += blockDim.x) s_wq[e] = M.wq1[e];
  for (uint32_t e = threadIdx.x; e < c1; e += blockDim.x) s_b1[e] = M.b1[e];
  const uint32_t total = HERRO_ROWS * kw * c1;
  for (uint32_t tk = 0; tk < TOKB; tk++) {
    const uint32_t n = blockIdx.x * TOKB + tk;
    if (n >= n_tok) break;
    const uint32_t b = S.tok_win[n];
    const int32_t l = (int32_t)S.tok_row[n];
    const int32_t len = (int32_t)B.len[b], lmax = (int32_t)B.lmax[b];
    const uint8_t* pb = B.planes_b + B.plane_off[b];
    const uint8_t* pq = B.planes_q + B.plane_off[b];
    const uint32_t ld = B.plane_ld[b];
    const uint8_t* rq = (B.rf_q && P <= 8) ? B.rf_q + ((B.rf_base ? B.rf_base[b] : B.out_off[b]) + (n - B.tok_off[b])) * HERRO_ROWS * 16 : nullptr;   // the token's receptive fields, compact: per read row 8 tokens + 8 qualities (k_rfq)
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < HERRO_ROWS * P; e += blockDim.x) {
      const uint32_t r = e / P;
      const int32_t q = l - 2 * (int32_t)h + (int32_t)(e % P);
      uint32_t tok = 255u;
      float qn = 0.f;
      if (q >= 0 && q < lmax) {
        if (q < len) {
          tok = rq ? rq[r * 16 + e % P] : pb[(uint64_t)r * ld + q];
          qn = norm_qual(rq ? rq[r * 16 + 8 + e % P] : pq[(uint64_t)r * ld + q]);
        } else {  // batch padding (inference.rs:86-97)
          tok = TOK_PAD;
          qn = norm_qual(126u);
        }
      }
      s_tok[e] = tok;
      s_qn[e] = qn;
    }
    __syncthreads();
    const uint64_t ob = (uint64_t)n * total;
    for (uint32_t e4 = threadIdx.x * 4; e4 < total; e4 += blockDim.x * 4) {  // 4 consecutive channels per thread
      const uint32_t c = e4 % c1, dl = (e4 / c1) % kw, r = e4 / (c1 * kw);
      const int32_t pos = l + (int32_t)dl - (int32_t)h;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pos >= 0 && pos < lmax) {  // outside: conv2's zero padding
        v = *reinterpret_cast<const float4*>(s_b1 + c);
        for (uint32_t t = 0; t < kw; t++) {
          const uint32_t pi = dl + t;
          const uint32_t tok = s_tok[r * P + pi];
          if (tok != 255u) {
            const float4 tv = *reinterpret_cast<const float4*>(s_t1 + (t * 12 + tok) * c1 + c);
            const float4 wv = *reinterpret_cast<const float4*>(s_wq + t * c1 + c);
            const float qn = s_qn[r * P + pi];
            v.x += tv.x + wv.x * qn; v.y += tv.y + wv.y * qn; v.z += tv.z + wv.z * qn; v.w += tv.w + wv.w * qn;
          }
        }
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      }
      const float f[4] = {v.x, v.y, v.z, v.w};
      uint16_t hb[4], lb[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        hb[q] = f32_to_bf16_rne(f[q]);
        lb[q] = f32_to_bf16_rne(f[q] - bf16_to_f32(hb[q]));
      }
      *reinterpret_cast<uint2*>(S.y1_hi + ob + e4) = make_uint2(hb[0] | ((uint32_t)hb[1] << 16), hb[2] | ((uint32_t)hb[3] << 16));
      *reinterpret_cast<uint2*>(S.y1_lo + ob + e4) = make_uint2(lb[0] | ((uint32_t)lb[1] << 16), lb[2] | ((uint32_t)lb[3] << 16));
    }
  }
}

// C[M,N] = epi(A . W^T + bias) (+R) with A given as bf16 hi/lo planes and W as [N][K] hi/lo planes;
// 3 MFMAs per k-step and tile: al*bh + ah*bl + ah*bh.
static constexpr int GN = 64;
// TM = 128: 4 waves x (32 rows x 64 cols); TM = 64: 4 waves x (16 rows x 64 cols) — used when the 128-row
// grid would leave the chip under-filled.

// ---------------------------------------------------------------------------------------------------
// LDS-DMA GEMM (bf16x3).  Phase-mask measurements of the register-staged predecessor (global -> VGPR ->
// ds_write, two barriers per k-step) showed its cost was additive — loop skeleton + global-load wait + MFMA
// + epilogue, nothing overlapped.  Here tiles go global -> LDS with global_load_lds_dwordx4 (no staging VGPRs, no ds_write), three LDS
// buffers keep two k-tiles in flight, waits are counted (vmcnt never drains inside the loop) and there is
// ONE barrier per k-step.  Every wave stages the A rows it alone consumes plus a quarter of the B tile.
// LDS rows are 64 bytes (BK = 32); the DMA destination is lane-linear, so the bank swizzle of the
// fragment reads (chunk ^ (row>>1)&3) is applied on the per-lane SOURCE address (same involution).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

template <bool OUT_SPLIT, int TM>
__global__ __launch_bounds__(256) void k_gemm_g(const uint16_t* __restrict__ Ahi, const uint16_t* __restrict__ Alo,
                                                uint32_t lda, Weight W, float* C, uint16_t* Chi, uint16_t* Clo,
                                                uint32_t ldc, const float* R, uint32_t M, int relu, uint32_t gx, uint32_t gy) {
  constexpr int RI = TM / 64;              // 16-row MFMA tiles per wave
  constexpr int BS = (2 * TM + 2 * GN) * 32;  // u16 elements of one buffer: A hi, A lo, B hi, B lo tiles of 64-byte rows
  constexpr int NBUF = 3;
  constexpr int NP = 2 * RI + 2;           // DMA pieces (1 KiB each) a wave issues per k-tile
  __shared__ __attribute__((aligned(1024))) uint16_t s_raw[NBUF * BS];
  const uint32_t K = W.K, N = W.N;
  // XCD-aware tile order (8 XCDs with private L2s; workgroup b runs on XCD b % 8): every XCD owns a
  // contiguous range of row tiles and walks (row tile, column tile) with the column fastest, so all
  // column tiles that share an A row tile hit the same L2 instead of pulling A through the fabric 8x.
  const uint32_t xcd = blockIdx.x & 7u, iin = blockIdx.x >> 3;
  const uint32_t rpx = (gy + 7u) / 8u;
  const uint32_t rt = xcd * rpx + iin / gx, ct = iin % gx;
  if (iin / gx >= rpx || rt >= gy) return;
  const uint32_t m0 = rt * TM, n0 = ct * GN;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t fr = lane & 15, fc = lane >> 4;

  f32x4 acc[RI][4];
#pragma unroll
  for (int i = 0; i < RI; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias of this lane's four output columns, fetched once up front (as 16 predicated loads in the epilogue
  // they were 16 serialized round trips)
  float bs[4];
#pragma unroll
  for (int j = 0; j < 4; j++) bs[j] = W.bias ? W.bias[min(n0 + j * 16 + (lane & 15), N - 1)] : 0.f;

  // staging plan: lane l of a piece fills row (l >> 2), 16-byte slot (l & 3); rows past M / N are clamped
  // (their products land in accumulators that are never stored)
  const uint32_t lr = lane >> 2, lc = lane & 3;
  const uint16_t* src[NP];
  uint32_t dst[NP];  // byte offset of the piece inside a buffer (wave-uniform)
#pragma unroll
  for (int i = 0; i < RI; i++) {
    const uint32_t row0 = wave * (TM / 4) + i * 16, row = row0 + lr;
    const uint32_t ch = lc ^ ((row >> 1) & 3u);
    const uint64_t g = (uint64_t)min(m0 + row, M - 1) * lda + ch * 8;
    src[2 * i] = Ahi + g;
    src[2 * i + 1] = Alo + g;
    dst[2 * i] = row0 * 64;
    dst[2 * i + 1] = TM * 64 + row0 * 64;
  }
  {
    const uint32_t row0 = wave * 16, row = row0 + lr;
    const uint32_t ch = lc ^ ((row >> 1) & 3u);
    const uint64_t g = (uint64_t)min(n0 + row, N - 1) * K + ch * 8;
    src[2 * RI] = W.hi + g;
    src[2 * RI + 1] = W.lo + g;
    dst[2 * RI] = 2 * TM * 64 + row0 * 64;
    dst[2 * RI + 1] = 2 * TM * 64 + GN * 64 + row0 * 64;
  }
  const uint32_t lds_base = (uint32_t)(uintptr_t)s_raw;
  auto stage = [&](uint32_t kt, uint32_t buf) {
    const uint32_t b0 = lds_base + buf * (BS * 2);
#pragma unroll
    for (int p = 0; p < NP; p++) glds16(src[p] + kt * 32, __builtin_amdgcn_readfirstlane(b0 + dst[p]));
  };
  auto compute = [&](uint32_t buf) {
    const uint16_t* s_ah = s_raw + buf * BS;
    const uint16_t* s_al = s_ah + TM * 32;
    const uint16_t* s_bh = s_al + TM * 32;
    const uint16_t* s_bl = s_bh + GN * 32;
    bf16x8 ah[RI], al[RI], bh[4], bl[4];
#pragma unroll
    for (int i = 0; i < RI; i++) {
      const uint32_t ar = wave * (TM / 4) + i * 16 + fr;
      const uint32_t o = ar * 32 + (fc ^ ((ar >> 1) & 3u)) * 8;
      ah[i] = *reinterpret_cast<const bf16x8*>(s_ah + o);
      al[i] = *reinterpret_cast<const bf16x8*>(s_al + o);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t br = j * 16 + fr;
      const uint32_t o = br * 32 + (fc ^ ((br >> 1) & 3u)) * 8;
      bh[j] = *reinterpret_cast<const bf16x8*>(s_bh + o);
      bl[j] = *reinterpret_cast<const bf16x8*>(s_bl + o);
    }
#pragma unroll
    for (int i = 0; i < RI; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
      }
  };

  const uint32_t nk = K / 32;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  uint32_t buf = 0, nbuf = 2;  // buffer of tile k / of tile k+2
  for (uint32_t k = 0; k < nk; k++) {
    // this wave's pieces of tile k have landed (tile k+1 may stay in flight) ...
    if (k + 1 < nk) wait_vmcnt<NP>(); else wait_vmcnt<0>();
    // ... and so have everybody else's; also every wave is done reading tile k-1, whose buffer tile k+2 reuses
    __builtin_amdgcn_s_barrier();
    if (k + 2 < nk) stage(k + 2, nbuf);
    compute(buf);
    buf = buf == NBUF - 1 ? 0 : buf + 1;
    nbuf = nbuf == NBUF - 1 ? 0 : nbuf + 1;
  }
  __syncthreads();  // tiles are dead from here on (the epilogue reuses the LDS)

  if constexpr (OUT_SPLIT) {
    constexpr int OLD = GN + 8, WR = TM / 4;
    static_assert(4 * WR * OLD <= NBUF * BS, "staging tile must fit the operand tiles");
    uint16_t* so = s_raw + wave * WR * OLD;
#pragma unroll
    for (int plane = 0; plane < 2; plane++) {
#pragma unroll
      for (int i = 0; i < RI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t nl = j * 16 + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            float v = acc[i][j][r] + bs[j];
            v = apply_act(v, relu);
            const uint16_t hb = f32_to_bf16_rne(v);
            so[(i * 16 + (lane >> 4) * 4 + r) * OLD + nl] = plane == 0 ? hb : f32_to_bf16_rne(v - bf16_to_f32(hb));
          }
        }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes have landed (wave-private region)
      __builtin_amdgcn_wave_barrier();
      uint16_t* dstp = plane == 0 ? Chi : Clo;
#pragma unroll
      for (int it = 0; it < WR / 8; it++) {  // WR rows x 8 chunks of 16 B
        const uint32_t ch = lane + it * 64, rr = ch >> 3, c8 = (ch & 7) * 8;
        const uint32_t m = m0 + wave * WR + rr, n = n0 + c8;
        if (m < M && n < N) *reinterpret_cast<uint4*>(dstp + (uint64_t)m * ldc + n) = *reinterpret_cast<const uint4*>(so + rr * OLD + c8);
      }
      __builtin_amdgcn_wave_barrier();
    }
  } else {
    // residual rows are fetched branch-free (clamped addresses) so the loads are all in flight together
    // (no ReLU between GEMM and residual anywhere in this model; the general order is kept below)
    if (R && !relu) {
#pragma unroll
      for (int i = 0; i < RI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t n = min(n0 + j * 16 + (lane & 15), N - 1);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const uint32_t m = min(m0 + wave * (TM / 4) + i * 16 + (lane >> 4) * 4 + r, M - 1);
            acc[i][j][r] += R[(uint64_t)m * ldc + n];
          }
        }
    }
#pragma unroll
    for (int i = 0; i < RI; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t n = n0 + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t m = m0 + wave * (TM / 4) + i * 16 + (lane >> 4) * 4 + r;
          if (m < M && n < N) {
            float v = acc[i][j][r] + bs[j];
            if (relu) {
              v = apply_act(v, relu);
              if (R) v += R[(uint64_t)m * ldc + n];
            }
            C[(uint64_t)m * ldc + n] = v;
          }
        }
      }
  }
}

// Full-width variant for N = 256 outputs (the FC layer: K = 3968): one workgroup computes 128 rows x ALL 256
// columns, so the big A operand (y2: 16 KB per token) is pulled through L2 once instead of once per
// 64-column tile (4x).  8 waves as 2 x 4, wave tile 64 x 64 (4 x 4 MFMA tiles), three LDS buffers of
// A 128x32 + B 256x32 (hi, lo) = 48 KB each, LDS-DMA staging (6 pieces of 1 KiB per wave and k-step), one
// barrier per k-step.  Same arithmetic as k_gemm_g.
template <bool OUT_SPLIT>
__global__ __launch_bounds__(512) void k_gemm_g256(const uint16_t* __restrict__ Ahi, const uint16_t* __restrict__ Alo,
                                                   uint32_t lda, Weight W, float* C, uint16_t* Chi, uint16_t* Clo,
                                                   uint32_t ldc, const float* R, uint32_t M, int relu) {
  constexpr int TMX = 128, TNX = 256, NBUF = 3, NP = 6;
  constexpr int BS = (2 * TMX + 2 * TNX) * 32;  // u16 elements of one buffer
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_g256[];
  uint16_t* s_raw = reinterpret_cast<uint16_t*>(smem_g256);
  const uint32_t K = W.K;
  const uint32_t m0 = blockIdx.x * TMX;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t fr = lane & 15, fc = lane >> 4;
  const uint32_t wr = wave >> 2, wc = wave & 3;  // wave tile: rows 64 wr.., columns 64 wc..

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bs[4];
#pragma unroll
  for (int j = 0; j < 4; j++) bs[j] = W.bias ? W.bias[wc * 64 + j * 16 + (lane & 15)] : 0.f;

  // staging: 16 A pieces (8 row groups x hi/lo) + 32 B pieces (16 row groups x hi/lo) of 16 rows each;
  // wave w takes A piece pair w (rows 16w..) and B piece pairs 2w, 2w+1
  const uint32_t lr = lane >> 2, lc = lane & 3;
  const uint16_t* src[NP];
  uint32_t dst[NP];
  {
    const uint32_t row0 = wave * 16, row = row0 + lr;
    const uint64_t g = (uint64_t)min(m0 + row, M - 1) * lda + (lc ^ ((row >> 1) & 3u)) * 8;
    src[0] = Ahi + g; src[1] = Alo + g;
    dst[0] = row0 * 64; dst[1] = TMX * 64 + row0 * 64;
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t row0 = (wave * 2 + h) * 16, row = row0 + lr;
    const uint64_t g = (uint64_t)row * K + (lc ^ ((row >> 1) & 3u)) * 8;
    src[2 + 2 * h] = W.hi + g; src[3 + 2 * h] = W.lo + g;
    dst[2 + 2 * h] = 2 * TMX * 64 + row0 * 64; dst[3 + 2 * h] = 2 * TMX * 64 + TNX * 64 + row0 * 64;
  }
  const uint32_t lds_base = (uint32_t)(uintptr_t)s_raw;
  auto stage = [&](uint32_t kt, uint32_t buf) {
    const uint32_t b0 = lds_base + buf * (BS * 2);
#pragma unroll
    for (int p = 0; p < NP; p++) glds16(src[p] + kt * 32, __builtin_amdgcn_readfirstlane(b0 + dst[p]));
  };
  auto compute = [&](uint32_t buf) {
    const uint16_t* s_ah = s_raw + buf * BS;
    const uint16_t* s_al = s_ah + TMX * 32;
    const uint16_t* s_bh = s_al + TMX * 32;
    const uint16_t* s_bl = s_bh + TNX * 32;
    bf16x8 ah[4], al[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t ar = wr * 64 + i * 16 + fr;
      const uint32_t o = ar * 32 + (fc ^ ((ar >> 1) & 3u)) * 8;
      ah[i] = *reinterpret_cast<const bf16x8*>(s_ah + o);
      al[i] = *reinterpret_cast<const bf16x8*>(s_al + o);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t br = wc * 64 + j * 16 + fr;
      const uint32_t o = br * 32 + (fc ^ ((br >> 1) & 3u)) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s_bh + o);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s_bl + o);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
      }
    }
  };
  const uint32_t nk = K / 32;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  uint32_t buf = 0, nbuf = 2;
  for (uint32_t k = 0; k < nk; k++) {
    if (k + 1 < nk) wait_vmcnt<NP>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (k + 2 < nk) stage(k + 2, nbuf);
    compute(buf);
    buf = buf == NBUF - 1 ? 0 : buf + 1;
    nbuf = nbuf == NBUF - 1 ? 0 : nbuf + 1;
  }
  // epilogue (f32 output, optional ReLU / residual); OUT_SPLIT is not needed by any caller of this shape
  static_assert(!OUT_SPLIT, "only the f32 epilogue is implemented");
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t n = wc * 64 + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t m = m0 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (m < M) {
          float v = acc[i][j][r] + bs[j];
          v = apply_act(v, relu);
          if (R) v += R[(uint64_t)m * ldc + n];
          C[(uint64_t)m * ldc + n] = v;
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------
// K = 256 GEMM with the weights resident in registers (the layout that halved the conv kernel): a
// workgroup owns a 128-channel slab of W (wave w: 32 channels, hi / lo fragments of all 8 k-steps =
// 128 VGPRs, loaded once) and walks token tiles of 128 persistently.  Only the activation tile moves:
// global -> LDS by LDS-DMA, three buffers, the pipeline runs straight across tile boundaries, one
// barrier per k-step.  MFMA roles are swapped (weights = A operand) and the channel order of the wave's
// two 16-channel tiles is permuted so that a lane ends up with 8 consecutive output channels of one
// token: results leave as 16-byte stores straight from the accumulators.
// L2 -> CU traffic per GEMM: A x (N / 128) + W once per workgroup, against A x (N / 64) + W x (M / 128)
// for the tiled kernel above, which measured ~10 TB/s of exactly that traffic and nothing else.
// ---------------------------------------------------------------------------------------------------
template <bool OUT_SPLIT>
__global__ __launch_bounds__(256, 2) void k_gemm_w(const uint16_t* __restrict__ Ahi, const uint16_t* __restrict__ Alo,
                                                   uint32_t lda, Weight W, float* C, uint16_t* Chi, uint16_t* Clo,
                                                   uint32_t ldc, const float* R, uint32_t M, int relu, uint32_t ns,
                                                   uint32_t ntiles) {
  constexpr int KS = 8, TP = 128, NBUF = 3, NP = 4;
  constexpr int BS = 2 * TP * 32;  // u16 elements of one buffer: hi tile, lo tile of 64-byte rows
  __shared__ __attribute__((aligned(1024))) uint16_t s_x[NBUF * BS];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t fr = lane & 15, fg = lane >> 4;
  const uint32_t slab = blockIdx.x % ns, tl = blockIdx.x / ns, tstride = gridDim.x / ns;
  if (tl >= ntiles) return;
  const uint32_t c0 = slab * 128 + wave * 32;

  bf16x8 wh[KS][2], wl[KS][2];
#pragma unroll
  for (int jt = 0; jt < 2; jt++) {
    const uint32_t ch = c0 + 8 * (fr >> 2) + 4 * jt + (fr & 3);  // lane group g ends up with channels c0+8g..+7
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      wh[ks][jt] = *reinterpret_cast<const bf16x8*>(W.hi + (uint64_t)ch * 256 + ks * 32 + fg * 8);
      wl[ks][jt] = *reinterpret_cast<const bf16x8*>(W.lo + (uint64_t)ch * 256 + ks * 32 + fg * 8);
    }
  }
  float bias8[8];
#pragma unroll
  for (int q = 0; q < 8; q++) bias8[q] = W.bias ? W.bias[c0 + 8 * fg + q] : 0.f;

  // staging plan: wave w moves rows 32w..32w+31 of the hi and lo tiles (4 pieces of 1 KiB per k-step);
  // lane l of a piece fills row (l >> 2), 16-byte slot (l & 3), swizzle applied on the source address
  const uint32_t lr = lane >> 2, lc = lane & 3;
  const uint32_t lds_base = (uint32_t)(uintptr_t)s_x;
  uint64_t off_cur[2], off_nxt[2];
  auto tile_offs = [&](uint32_t t, uint64_t (&o)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const uint32_t row = wave * 32 + i * 16 + lr;
      o[i] = (uint64_t)min(t * TP + row, M - 1) * lda + (lc ^ ((row >> 1) & 3u)) * 8;
    }
  };
  auto stage = [&](const uint64_t (&o)[2], uint32_t ks, uint32_t buf) {
    const uint32_t b0 = lds_base + buf * (BS * 2) + wave * 32 * 64;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      glds16(Ahi + o[i] + ks * 32, __builtin_amdgcn_readfirstlane(b0 + i * 16 * 64));
      glds16(Alo + o[i] + ks * 32, __builtin_amdgcn_readfirstlane(b0 + TP * 64 + i * 16 * 64));
    }
  };

  f32x4 acc[8][2];
#pragma unroll
  for (int pt = 0; pt < 8; pt++)
#pragma unroll
    for (int jt = 0; jt < 2; jt++) acc[pt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};

  tile_offs(tl, off_cur);
  stage(off_cur, 0, 0);
  stage(off_cur, 1, 1);
  uint32_t buf = 0, nbuf = 2;  // buffer of the current step / of the step two ahead
  for (uint32_t t = tl; t < ntiles; t += tstride) {
    const bool more = t + tstride < ntiles;
    if (more) tile_offs(t + tstride, off_nxt);
    auto step = [&](auto ksc) {
      constexpr int ks = decltype(ksc)::value;
      // this wave's pieces of the current step have landed (the next step's may stay in flight) ...
      if (ks < KS - 1 || more) wait_vmcnt<NP>(); else wait_vmcnt<0>();
      // ... and everybody else's; every wave is also done reading the buffer the step two ahead reuses
      __builtin_amdgcn_s_barrier();
      if (ks + 2 < KS) stage(off_cur, ks + 2, nbuf);
      else if (more) stage(off_nxt, ks + 2 - KS, nbuf);
      const uint16_t* xh = s_x + buf * BS;
      const uint16_t* xl = xh + TP * 32;
#pragma unroll
      for (int pt = 0; pt < 8; pt++) {
        const uint32_t pr = pt * 16 + fr;
        const uint32_t o = pr * 32 + (fg ^ ((pr >> 1) & 3u)) * 8;
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(xh + o);
        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(xl + o);
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks][jt], bh, acc[pt][jt], 0, 0, 0);
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][jt], bl, acc[pt][jt], 0, 0, 0);
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][jt], bh, acc[pt][jt], 0, 0, 0);
        }
      }
      buf = buf == NBUF - 1 ? 0 : buf + 1;
      nbuf = nbuf == NBUF - 1 ? 0 : nbuf + 1;
    };
    step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{}); step(std::integral_constant<int, 3>{});
    step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
    step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});

    // epilogue: lane = token (fr) x 8 consecutive channels (c0 + 8 fg ..)
#pragma unroll
    for (int pt = 0; pt < 8; pt++) {
      const uint32_t m = t * TP + pt * 16 + fr;
      const uint64_t o = (uint64_t)min(m, M - 1) * ldc + c0 + 8 * fg;
      float v[8];
#pragma unroll
      for (int jt = 0; jt < 2; jt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          v[jt * 4 + r] = acc[pt][jt][r] + bias8[jt * 4 + r];
          acc[pt][jt][r] = 0.f;
        }
      if (relu) {
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = apply_act(v[q], relu);
      }
      if constexpr (OUT_SPLIT) {
        uint4 hv, lv;
        split2(v[0], v[1], hv.x, lv.x);
        split2(v[2], v[3], hv.y, lv.y);
        split2(v[4], v[5], hv.z, lv.z);
        split2(v[6], v[7], hv.w, lv.w);
        if (m < M) {
          *reinterpret_cast<uint4*>(Chi + o) = hv;
          *reinterpret_cast<uint4*>(Clo + o) = lv;
        }
      } else {
        if (R) {
          const float4 r0 = *reinterpret_cast<const float4*>(R + o), r1 = *reinterpret_cast<const float4*>(R + o + 4);
          v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w;
          v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
        }
        if (m < M) {
          *reinterpret_cast<float4*>(C + o) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(C + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    }
    if (more) { off_cur[0] = off_nxt[0]; off_cur[1] = off_nxt[1]; }
  }
}

// ---------------------------------------------------------------------------------------------------
// conv1 fused into the conv2 GEMM (kw = 3, c1 = 64, c2 = 128).  GEMM rows are (token, read row) pairs;
// their conv1 activations (3 taps x 64 channels = the K axis, 192) are computed on the fly from the
// window's token / quality planes straight into an LDS tile, so the [N*31, 192] tensor never exists in
// HBM.  Phase masks on the first version of this kernel (one 128-pair tile per workgroup, weights
// re-staged through LDS every k-step) showed 40 % of its time in the skeleton (weight staging +
// barriers) and 28 % in the latency chain of the input gather, so this one is built the other way round:
//   * persistent workgroups (2 per CU) walk the pair tiles;
//   * the conv2 weights never touch LDS: wave w owns output channels 32w..32w+31 and keeps their
//     hi / lo fragments for all 6 k-steps in 96 VGPRs, loaded once per workgroup;
//   * MFMA roles are swapped (weights = A operand, pairs = B operand), and the channel order inside the
//     wave's two 16-channel tiles is permuted so that a lane ends up with 8 CONSECUTIVE channels of one
//     pair: y2 leaves as 16-byte stores straight from the accumulators, no LDS transpose;
//   * the input patch of the next tile (and the token records of the one after) is prefetched into
//     registers while the current tile computes;
//   * the activation tile is double-buffered: one barrier per k-step.
// ---------------------------------------------------------------------------------------------------
static constexpr int FC2 = 128;
static constexpr int CLD = 32;  // unpadded 64-byte LDS rows, 16-byte chunks XOR-swizzled by (row>>1)&3 (conflict-free b128 reads)
__device__ __forceinline__ uint32_t cswz(uint32_t row, uint32_t chunk) { return chunk ^ ((row >> 1) & 3u); }
static constexpr int CW_TP = 128;   // pairs per tile
static constexpr int CW_T1R = 13;   // token rows of the LDS table: 12 tokens + a zero row for cells outside the window
static constexpr size_t CW_SHM = (size_t)2 * 2 * CW_TP * CLD * 2 + (size_t)(3 * CW_T1R * 64 + 3 * 64 + 64) * 4 + (size_t)CW_TP * 8 * 4 +
                                 (size_t)CW_TP * 8 + (size_t)CW_TP * 4;

__global__ __launch_bounds__(256, 2) void k_conv_w(ModelDev M, BatchDev B, ModelScratch S, uint32_t n_rows, uint32_t n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* s_x = reinterpret_cast<uint16_t*>(smem);                 // [2 buffers][hi, lo][128][32]
  float* s_t1 = reinterpret_cast<float*>(s_x + 2 * 2 * CW_TP * CLD);  // [3][13][64]
  float* s_wq = s_t1 + 3 * CW_T1R * 64;                               // [3][64]
  float* s_b1 = s_wq + 3 * 64;                                        // [64]
  float* s_qn = s_b1 + 64;                                            // [128][8] normalised quality (5 used)
  uint8_t* s_tok = reinterpret_cast<uint8_t*>(s_qn + CW_TP * 8);      // [128][8] token, 12 = outside
  uint8_t* s_val = s_tok + CW_TP * 8;                                 // [128][4] conv1 position inside [0,lmax)?
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t fr = lane & 15, fg = lane >> 4;

  // ---- once per workgroup: tables, weight fragments, bias
  for (uint32_t e = tid; e < 3 * CW_T1R * 64; e += 256) {
    const uint32_t t = e / (CW_T1R * 64), rem = e % (CW_T1R * 64), tok = rem / 64, c = rem % 64;
    s_t1[e] = tok < 12 ? M.t1[(t * 12 + tok) * 64 + c] : 0.f;
  }
  for (uint32_t e = tid; e < 3 * 64; e += 256) s_wq[e] = M.wq1[e];
  for (uint32_t e = tid; e < 64; e += 256) s_b1[e] = M.b1[e];
  const Weight& W = M.conv2;
  const uint32_t c0 = wave * 32;
  bf16x8 wh[6][2], wl[6][2];
#pragma unroll
  for (int jt = 0; jt < 2; jt++) {
    // MFMA row i of tile jt <-> channel c0 + 8*(i>>2) + 4*jt + (i&3): lane group g then holds channels c0+8g..+7
    const uint32_t ch = c0 + 8 * (fr >> 2) + 4 * jt + (fr & 3);
#pragma unroll
    for (int ks = 0; ks < 6; ks++) {
      wh[ks][jt] = *reinterpret_cast<const bf16x8*>(W.hi + (uint64_t)ch * 192 + ks * 32 + fg * 8);
      wl[ks][jt] = *reinterpret_cast<const bf16x8*>(W.lo + (uint64_t)ch * 192 + ks * 32 + fg * 8);
    }
  }
  float bias8[8];
#pragma unroll
  for (int q = 0; q < 8; q++) bias8[q] = W.bias[c0 + 8 * fg + q];

  // ---- gather: threads 0..127 fetch the 5 tokens of pair tid, threads 128..255 its 5 qualities
  const uint32_t grr = tid & 127u;
  const bool gq = tid >= 128;
  const bool rfq = B.rf_q != nullptr;   // tokens and qualities from the compact receptive-field records (16 bytes per pair: 8 tokens, 8 qualities)
  const uint8_t* gplane = rfq ? B.rf_q : (gq ? B.planes_q : B.planes_b);
  struct PairMeta { uint64_t rowbase; uint32_t tok_row, len, lmax; };  // lmax = 0: no such pair
  auto load_meta = [&](uint32_t tile) -> PairMeta {
    const uint32_t m = tile * CW_TP + grr;
    PairMeta r{0, 0, 0, 0};
    if (tile < n_tiles && m < n_rows) {
      const TokMeta tm = S.tok_meta[m / HERRO_ROWS];
      r.rowbase = tm.plane_off + (uint64_t)(m % HERRO_ROWS) * tm.plane_ld;  // byte offset of the read row
      if (rfq) r.rowbase = ((uint64_t)tm.rf_idx * HERRO_ROWS + m % HERRO_ROWS) * 16 + (gq ? 8u : 0u) - (uint64_t)(int64_t)((int32_t)tm.tok_row - 2);   // + q = record byte q - (tok_row - 2)
      r.tok_row = tm.tok_row;
      r.len = tm.len;
      r.lmax = tm.lmax;
    }
    return r;
  };
  auto load_cells = [&](const PairMeta& mt, uint32_t (&g)[5]) {
#pragma unroll
    for (int pi = 0; pi < 5; pi++) {
      const int32_t q = (int32_t)mt.tok_row - 2 + pi;
      uint32_t v = gq ? 0xffffffffu : 12u;  // outside [0, lmax): contributes nothing
      if (q >= 0 && q < (int32_t)mt.lmax) v = q < (int32_t)mt.len ? (uint32_t)gplane[mt.rowbase + (uint32_t)q] : (gq ? 126u : (uint32_t)TOK_PAD);
      g[pi] = v;
    }
  };
  uint32_t g[5];
  PairMeta mcur = load_meta(blockIdx.x);
  load_cells(mcur, g);
  PairMeta mnext = load_meta(blockIdx.x + gridDim.x);

  f32x4 acc[8][2];
  const uint32_t arow = tid >> 3, kk = (tid & 7) * 4;  // activation items: rows arow + 32*it, channels kk..kk+3 of the k-step
  __syncthreads();  // tables complete

  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t m0 = tile * CW_TP;
    // patch of this tile: registers -> LDS
    if (!gq) {
      *reinterpret_cast<uint2*>(s_tok + grr * 8) = make_uint2(g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24), g[4]);
      uint32_t vb = 0;
#pragma unroll
      for (int dl = 0; dl < 3; dl++) {
        const int32_t pos = (int32_t)mcur.tok_row + dl - 1;
        if (pos >= 0 && pos < (int32_t)mcur.lmax) vb |= 1u << (8 * dl);  // else: conv2's zero padding
      }
      *reinterpret_cast<uint32_t*>(s_val + grr * 4) = vb;
    } else {
      float qn[5];
#pragma unroll
      for (int pi = 0; pi < 5; pi++) qn[pi] = g[pi] != 0xffffffffu ? norm_qual(g[pi]) : 0.f;
      *reinterpret_cast<float4*>(s_qn + grr * 8) = make_float4(qn[0], qn[1], qn[2], qn[3]);
      s_qn[grr * 8 + 4] = qn[4];
    }
    __syncthreads();
    // prefetch: cells of the next tile, token records of the one after
    mcur = mnext;
    load_cells(mcur, g);
    mnext = load_meta(tile + 2 * gridDim.x);

#pragma unroll
    for (int pt = 0; pt < 8; pt++)
#pragma unroll
      for (int jt = 0; jt < 2; jt++) acc[pt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto gen = [&](auto ksc) {  // conv1 (+BN folded) + ReLU of 128 pairs x 32 channels of k-step ks -> buffer ks & 1
      constexpr int ks = decltype(ksc)::value;
      constexpr int dl = ks >> 1, cb = (ks & 1) * 32;
      uint16_t* xh = s_x + (ks & 1) * (2 * CW_TP * CLD);
      uint16_t* xl = xh + CW_TP * CLD;
      const uint32_t c = cb + kk;
      const float4 b1v = *reinterpret_cast<const float4*>(s_b1 + c);
      float4 wq[3];
#pragma unroll
      for (int t = 0; t < 3; t++) wq[t] = *reinterpret_cast<const float4*>(s_wq + t * 64 + c);
#pragma unroll
      for (int it = 0; it < 4; it++) {
        const uint32_t rr = arow + it * 32;
        const uint2 tk = *reinterpret_cast<const uint2*>(s_tok + rr * 8);
        const uint64_t tk64 = (uint64_t)tk.x | ((uint64_t)tk.y << 32);
        float4 v = b1v;
#pragma unroll
        for (int t = 0; t < 3; t++) {
          const uint32_t tok = (uint32_t)(tk64 >> (8 * (dl + t))) & 0xffu;
          const float4 tv = *reinterpret_cast<const float4*>(s_t1 + (t * CW_T1R + tok) * 64 + c);
          const float qn = s_qn[rr * 8 + dl + t];
          v.x += tv.x + wq[t].x * qn; v.y += tv.y + wq[t].y * qn; v.z += tv.z + wq[t].z * qn; v.w += tv.w + wq[t].w * qn;
        }
        const bool ok = s_val[rr * 4 + dl] != 0;
        v.x = ok ? fmaxf(v.x, 0.f) : 0.f; v.y = ok ? fmaxf(v.y, 0.f) : 0.f;
        v.z = ok ? fmaxf(v.z, 0.f) : 0.f; v.w = ok ? fmaxf(v.w, 0.f) : 0.f;
        uint32_t h01, l01, h23, l23;
        split2(v.x, v.y, h01, l01);
        split2(v.z, v.w, h23, l23);
        const uint32_t o = rr * CLD + cswz(rr, kk >> 3) * 8 + (kk & 7);
        *reinterpret_cast<uint2*>(xh + o) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(xl + o) = make_uint2(l01, l23);
      }
    };
    auto mma = [&](auto ksc) {
      constexpr int ks = decltype(ksc)::value;
      const uint16_t* xh = s_x + (ks & 1) * (2 * CW_TP * CLD);
      const uint16_t* xl = xh + CW_TP * CLD;
#pragma unroll
      for (int pt = 0; pt < 8; pt++) {
        const uint32_t pr = pt * 16 + fr;
        const uint32_t o = pr * CLD + cswz(pr, fg) * 8;
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(xh + o);
        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(xl + o);
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks][jt], bh, acc[pt][jt], 0, 0, 0);
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][jt], bl, acc[pt][jt], 0, 0, 0);
          acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][jt], bh, acc[pt][jt], 0, 0, 0);
        }
      }
    };
    using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>; using K3 = std::integral_constant<int, 3>;
    using K4 = std::integral_constant<int, 4>; using K5 = std::integral_constant<int, 5>;
    gen(K0{});
    __syncthreads();
    gen(K1{}); mma(K0{}); __syncthreads();
    gen(K2{}); mma(K1{}); __syncthreads();
    gen(K3{}); mma(K2{}); __syncthreads();
    gen(K4{}); mma(K3{}); __syncthreads();
    gen(K5{}); mma(K4{}); __syncthreads();
    mma(K5{});
    // epilogue: + bias (BN folded), ReLU, split; lane = pair (fr) x 8 consecutive channels (c0 + 8 fg ..)
#pragma unroll
    for (int pt = 0; pt < 8; pt++) {
      const uint32_t m = m0 + pt * 16 + fr;
      float v[8];
#pragma unroll
      for (int jt = 0; jt < 2; jt++)
#pragma unroll
        for (int r = 0; r < 4; r++) v[jt * 4 + r] = fmaxf(acc[pt][jt][r] + bias8[jt * 4 + r], 0.f);
      uint4 hv, lv;
      split2(v[0], v[1], hv.x, lv.x);
      split2(v[2], v[3], hv.y, lv.y);
      split2(v[4], v[5], hv.z, lv.z);
      split2(v[6], v[7], hv.w, lv.w);
      if (m < n_rows) {
        const uint64_t o = (uint64_t)m * FC2 + c0 + 8 * fg;
        *reinterpret_cast<uint4*>(S.y2_hi + o) = hv;
        *reinterpret_cast<uint4*>(S.y2_lo + o) = lv;
      }
    }
    __syncthreads();  // the last k-step's reads are done before the next tile overwrites the patch / buffer 1
  }
}

// The opt-in for more than 64 KB of dynamic LDS is a per-DEVICE function attribute: a process that drives one context per
// GPU must set it on every device it launches on, so the "done" set is keyed by (function, device).
static void opt_in_dynamic_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lk(mu);
  if (done.insert({fn, dev}).second) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <bool SPLIT, int TM>
static void gemm_launch(uint32_t gx, uint32_t gy, const uint16_t* Ahi, const uint16_t* Alo, uint32_t lda, const Weight& W,
                        float* C, uint16_t* Chi, uint16_t* Clo, uint32_t ldc, const float* R, uint32_t M, int relu,
                        hipStream_t st) {
  const dim3 grid(8u * ((gy + 7u) / 8u) * gx);  // 1-D, remapped inside the kernel
  hipLaunchKernelGGL((k_gemm_g<SPLIT, TM>), grid, dim3(256), 0, st, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, gx, gy);
}

static void gemm_s(const uint16_t* Ahi, const uint16_t* Alo, uint32_t lda, const Weight& W, float* C, uint16_t* Chi,
                   uint16_t* Clo, uint32_t ldc, const float* R, uint32_t M, int relu, hipStream_t st) {
  if (M == 0) return;
  // full-width tiles: A streams through L2 once.  Needs >= one 128-row tile per CU to fill the chip
  // (HERRO_G256_MIN_M overrides the threshold: the tests use it to cover the kernel with small inputs)
  static const uint32_t g256_min_m = getenv("HERRO_G256_MIN_M") ? (uint32_t)atoi(getenv("HERRO_G256_MIN_M")) : 128u * 256u;
  if (W.N == 256 && !Chi && W.K >= 1024 && W.K % 32 == 0 && M >= g256_min_m) {
    constexpr size_t shm = (size_t)3 * (2 * 128 + 2 * 256) * 32 * 2;
    opt_in_dynamic_lds(reinterpret_cast<const void*>(k_gemm_g256<false>), shm);
    hipLaunchKernelGGL(k_gemm_g256<false>, dim3((M + 127) / 128), dim3(512), shm, st, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu);
    return;
  }
  if (W.K == 256 && W.N % 128 == 0) {  // weights-in-registers kernel
    const uint32_t ns = W.N / 128, ntiles = (M + 127) / 128;
    const uint32_t per_slab = std::min<uint32_t>(ntiles, std::max<uint32_t>(512u / ns, 1u));
    if (Chi)
      hipLaunchKernelGGL(k_gemm_w<true>, dim3(per_slab * ns), dim3(256), 0, st, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, ns, ntiles);
    else
      hipLaunchKernelGGL(k_gemm_w<false>, dim3(per_slab * ns), dim3(256), 0, st, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, ns, ntiles);
    return;
  }
  const uint32_t gx = (W.N + GN - 1) / GN;
  const bool small = (uint64_t)gx * ((M + 127) / 128) < 1536;  // < ~6 workgroups per CU with 128-row tiles
  if (small) {
    const uint32_t gy = (M + 63) / 64;
    if (Chi) gemm_launch<true, 64>(gx, gy, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, st);
    else gemm_launch<false, 64>(gx, gy, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, st);
  } else {
    const uint32_t gy = (M + 127) / 128;
    if (Chi) gemm_launch<true, 128>(gx, gy, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, st);
    else gemm_launch<false, 128>(gx, gy, Ahi, Alo, lda, W, C, Chi, Clo, ldc, R, M, relu, st);
  }
}

// LayerNorm, one wave per row, output pre-split
// g == nullptr: no normalisation, the planes are the split of x itself (what a Post-LN layer's QKV GEMM reads).  xo != nullptr: the normalised row is also written
// back as f32 (Post-LN: the LayerNorm output IS the residual stream; xo may be x)
__global__ __launch_bounds__(256) void k_layernorm_s(const float* x, uint16_t* yh, uint16_t* yl, const float* g,
                                                     const float* b, uint32_t n_rows, uint32_t D, float eps, float* xo) {
  const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const float* xr = x + (uint64_t)row * D;
  if (!g) {
    for (uint32_t i = lane; i < D; i += 64) split_store(yh, yl, (uint64_t)row * D + i, xr[i]);
    return;
  }
  float s = 0.f;
  for (uint32_t i = lane; i < D; i += 64) s += xr[i];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  const float mean = s / (float)D;
  float v = 0.f;
  for (uint32_t i = lane; i < D; i += 64) {
    const float t = xr[i] - mean;
    v += t * t;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  const float rstd = 1.0f / sqrtf(v / (float)D + eps);
  for (uint32_t i = lane; i < D; i += 64) {
    const float y = (xr[i] - mean) * rstd * g[i] + b[i];
    split_store(yh, yl, (uint64_t)row * D + i, y);
    if (xo) xo[(uint64_t)row * D + i] = y;
  }
}

// Attention inside one window, all heads in one workgroup: 16 lanes per head, a lane owns one query
// at a time (the window's informative positions are the sequence; typically 10-30 tokens).  K and V
// rows are staged through LDS in chunks of KC keys with coalesced 16-byte loads; reads are broadcast
// within a head's 16 lanes.  Softmax is kept online in registers across chunks.  Output pre-split.
// blockIdx.y strides the blocks of 16 queries: this path is what windows above the fused stack's 64-token tile
// take, and one workgroup walking a 100-token window alone (7 query blocks x 7 key chunks, each a serial chain
// over 16 keys) took 330 us per layer for ten such windows.
static constexpr int KC = 16;
template <int DH>
__global__ __launch_bounds__(512) void k_attention_s(BatchDev B, ModelScratch S, uint32_t D) {   // 16 lanes per head: up to 32 heads (d_model 1024); was bounded at 128 threads = 8 heads, and a 16-head model failed to launch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_k = reinterpret_cast<float*>(smem);  // [KC][D]
  float* s_v = s_k + KC * D;                     // [KC][D]
  const uint32_t b = blockIdx.x, hd = threadIdx.x >> 4, ql = threadIdx.x & 15;
  const uint32_t t0 = B.tok_off[b], len = B.tok_off[b + 1] - t0;
  const float scale = 1.0f / sqrtf((float)DH);
  for (uint32_t i0 = blockIdx.y * 16; i0 < len; i0 += 16 * gridDim.y) {  // block-uniform trip count (barriers inside)
    const uint32_t i = i0 + ql;
    const bool act = i < len;
    float qr[DH], o[DH];
    if (act) {
      const float4* q4 = reinterpret_cast<const float4*>(S.qkv + (uint64_t)(t0 + i) * 3 * D + hd * DH);
#pragma unroll
      for (int d = 0; d < DH / 4; d++) {
        const float4 v = q4[d];
        qr[4 * d] = v.x * scale; qr[4 * d + 1] = v.y * scale; qr[4 * d + 2] = v.z * scale; qr[4 * d + 3] = v.w * scale;
      }
    }
#pragma unroll
    for (int d = 0; d < DH; d++) o[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (uint32_t j0 = 0; j0 < len; j0 += KC) {
      const uint32_t nk = min((uint32_t)KC, len - j0);
      __syncthreads();
      for (uint32_t e = threadIdx.x; e < nk * (D / 4); e += blockDim.x) {
        const uint32_t jr = e / (D / 4), c4 = e % (D / 4);
        const float4* src = reinterpret_cast<const float4*>(S.qkv + (uint64_t)(t0 + j0 + jr) * 3 * D + D);
        reinterpret_cast<float4*>(s_k)[jr * (D / 4) + c4] = src[c4];
        reinterpret_cast<float4*>(s_v)[jr * (D / 4) + c4] = src[D / 4 + c4];
      }
      __syncthreads();
      if (act) {
        for (uint32_t j = 0; j < nk; j++) {
          const float4* k4 = reinterpret_cast<const float4*>(s_k + j * D + hd * DH);
          const float4* v4 = reinterpret_cast<const float4*>(s_v + j * D + hd * DH);
          float sc = 0.f;
#pragma unroll
          for (int d = 0; d < DH / 4; d++) {
            const float4 kv = k4[d];
            sc = fmaf(qr[4 * d], kv.x, sc); sc = fmaf(qr[4 * d + 1], kv.y, sc);
            sc = fmaf(qr[4 * d + 2], kv.z, sc); sc = fmaf(qr[4 * d + 3], kv.w, sc);
          }
          const float mn = fmaxf(m, sc);
          const float alpha = expf(m - mn), pw = expf(sc - mn);
          l = l * alpha + pw;
#pragma unroll
          for (int d = 0; d < DH / 4; d++) {
            const float4 vv = v4[d];
            o[4 * d] = o[4 * d] * alpha + pw * vv.x; o[4 * d + 1] = o[4 * d + 1] * alpha + pw * vv.y;
            o[4 * d + 2] = o[4 * d + 2] * alpha + pw * vv.z; o[4 * d + 3] = o[4 * d + 3] * alpha + pw * vv.w;
          }
          m = mn;
        }
      }
    }
    if (act) {
      const float inv = 1.0f / l;
      const uint64_t ob = (uint64_t)(t0 + i) * D + hd * DH;
      uint32_t ph[DH / 2], pl[DH / 2];  // the head's DH outputs as packed bf16 pairs -> 16-byte stores
#pragma unroll
      for (int d = 0; d < DH; d += 2) {
        split2(o[d] * inv, o[d + 1] * inv, ph[d / 2], pl[d / 2]);
      }
#pragma unroll
      for (int d = 0; d < DH / 8; d++) {
        *reinterpret_cast<uint4*>(S.att_hi + ob + 8 * d) = make_uint4(ph[4 * d], ph[4 * d + 1], ph[4 * d + 2], ph[4 * d + 3]);
        *reinterpret_cast<uint4*>(S.att_lo + ob + 8 * d) = make_uint4(pl[4 * d], pl[4 * d + 1], pl[4 * d + 2], pl[4 * d + 3]);
      }
    }
  }
}


// ===================================================================================================
// The whole transformer stack in ONE kernel.
//
// Measured on the layer-by-layer pipeline (31 launches: LN, QKV, attention, proj, LN, FF1, FF2 per layer):
// every one of those ~20-50 us kernels pays a ~9 us launch/ramp floor, its phases (weights in, activations
// in, MFMA, stores out) run in lock-step over the chip and add up instead of overlapping, and all
// activations bounce through HBM between them.  Attention never crosses a window, so a tile of whole
// windows (<= 64 tokens) is independent through ALL layers: one workgroup takes a tile through the stack.
//   * 8 waves; the residual stream x[64][256] lives in registers (wave w: channels 32w..32w+31, a lane
//     holds 8 consecutive channels of 4 tokens) from the first LayerNorm to the logits;
//   * LayerNorm output, attention output and the FF hidden chunk are bf16 hi/lo planes in LDS
//     (XOR-swizzled 512-byte rows); nothing else touches memory;
//   * weights stream L2 -> registers as MFMA operand fragments (every weight element is fetched once per
//     workgroup); a wave owns 32 output channels of every GEMM;
//   * wave = head for attention: Q, K come out of the QKV GEMM already in MFMA operand layout (weights
//     as the A operand -> lane = token x 8 consecutive channels), V is produced with the MFMA roles
//     swapped so that it is already "transposed"; S^T = K Q^T, softmax and O^T = V^T P^T stay in
//     registers: the k-slot order (g, e) <-> token 32a + 16(e >> 2) + 4g + (e & 3) is the same for the
//     P^T and V^T fragments, so no data ever has to be transposed;
//   * FF1 -> ReLU -> FF2 is chunked over 256 hidden channels, the FF2 accumulator stays in registers.
// ===================================================================================================
static constexpr int LT = 64;  // tokens per tile
static constexpr size_t LAYERS_SHM = (size_t)4 * LT * 256 * 2 + 8 * LT * 4 + LT * 4;

__device__ __forceinline__ uint32_t lsw(uint32_t row, uint32_t chunk) { return row * 256 + ((chunk ^ (row & 15u)) << 3); }
__device__ __forceinline__ bf16x8 as_bf16x8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(bf16x8, make_uint4(a, b, c, d));
}
// 8 f32 values -> one MFMA k-chunk of 8 bf16, hi and lo planes
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  uint4 h, l;
  split2(v[0], v[1], h.x, l.x);
  split2(v[2], v[3], h.y, l.y);
  split2(v[4], v[5], h.z, l.z);
  split2(v[6], v[7], h.w, l.w);
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}

// acc[pt][jt] += W[32 channels at cb][K = 256 at kofs] x act[64 tokens][256] (LDS planes sh / sl).
// SWAP = false: weights are the MFMA A operand -> lane (token fr of tile pt) x channels cb + 8 fg + 4 jt + r.
// SWAP = true : activations are the A operand  -> lane (channel cb + 8 (fr>>2) + 4 jt + (fr&3)) x tokens 16 pt + 4 fg + r.
template <bool SWAP>
__device__ __forceinline__ void tile_gemm(const Weight& W, uint32_t cb, uint32_t kofs, const uint16_t* sh, const uint16_t* sl,
                                          uint32_t fr, uint32_t fg, f32x4 (&acc)[4][2]) {
  // weights arrive in two batches of 4 k-steps (64 VGPRs each): the full K at once does not fit next to the
  // attention fragments
  const uint32_t nks = W.K >> 5, lane = fg * 16 + fr;
  uint64_t wo[2];  // fragment-ordered planes (Weight::phi / plo): a wave's load is one contiguous KiB
#pragma unroll
  for (int jt = 0; jt < 2; jt++) wo[jt] = ((((uint64_t)(cb >> 5) * 2 + jt) * nks + (kofs >> 5)) * 64 + lane) * 8;
#pragma unroll
  for (int kb = 0; kb < 8; kb += 4) {
    bf16x8 wh[4][2], wl[4][2];
#pragma unroll
    for (int jt = 0; jt < 2; jt++)
#pragma unroll
      for (int k4 = 0; k4 < 4; k4++) {
        wh[k4][jt] = *reinterpret_cast<const bf16x8*>(W.phi + wo[jt] + (kb + k4) * 512);
        wl[k4][jt] = *reinterpret_cast<const bf16x8*>(W.plo + wo[jt] + (kb + k4) * 512);
      }
    // keep the 16 loads together and ahead of the MFMAs: left alone, the scheduler sinks every load next
    // to its first use (register pressure) and the kernel pays one L2 round trip per load
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k4 = 0; k4 < 4; k4++)
#pragma unroll
      for (int pt = 0; pt < 4; pt++) {
        const uint32_t o = lsw(pt * 16 + fr, (kb + k4) * 4 + fg);
        const bf16x8 xh = *reinterpret_cast<const bf16x8*>(sh + o);
        const bf16x8 xl = *reinterpret_cast<const bf16x8*>(sl + o);
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
          if (SWAP) {
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh[k4][jt], acc[pt][jt], 0, 0, 0);
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl[k4][jt], acc[pt][jt], 0, 0, 0);
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh[k4][jt], acc[pt][jt], 0, 0, 0);
          } else {
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[k4][jt], xh, acc[pt][jt], 0, 0, 0);
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[k4][jt], xl, acc[pt][jt], 0, 0, 0);
            acc[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[k4][jt], xh, acc[pt][jt], 0, 0, 0);
          }
        }
      }
  }
}

__global__ __launch_bounds__(512) void k_layers(ModelDev M, BatchDev B, ModelScratch S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* s_hh = reinterpret_cast<uint16_t*>(smem);  // LayerNorm output, hi / lo planes [64][256]
  uint16_t* s_hl = s_hh + LT * 256;
  uint16_t* s_ah = s_hl + LT * 256;                    // attention output, then FF hidden chunk
  uint16_t* s_al = s_ah + LT * 256;
  float* s_red = reinterpret_cast<float*>(s_al + LT * 256);      // [8 waves][64 tokens]
  uint32_t* s_win = reinterpret_cast<uint32_t*>(s_red + 8 * LT);  // [64] window of each token
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t fr = lane & 15, fg = lane >> 4;
  const uint32_t t0 = B.tile_tok0[blockIdx.x], nt = B.tile_tok0[blockIdx.x + 1] - t0;
  const uint32_t cw = wave * 32;  // this wave's channel slab of every 256-wide GEMM output
  const float eps = M.h.ln_eps;

  if (tid < LT) s_win[tid] = tid < nt ? S.tok_win[t0 + tid] : 0xffffff00u + tid;  // padding slots: a window of their own
  float x[4][8];

  // LayerNorm of the register-resident x over the 256 channels (8 waves x 4 lane groups x 8 registers);
  // two-pass like the unfused kernel; result goes to the s_hh / s_hl planes
  auto layer_norm = [&](const float* __restrict__ g, const float* __restrict__ b) {
    float mean[4], rstd[4];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll
      for (int pt = 0; pt < 4; pt++) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const float d = pass == 0 ? x[pt][q] : x[pt][q] - mean[pt];
          s += pass == 0 ? d : d * d;
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (fg == 0) s_red[wave * LT + pt * 16 + fr] = s;
      }
      __syncthreads();
#pragma unroll
      for (int pt = 0; pt < 4; pt++) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 8; w++) s += s_red[w * LT + pt * 16 + fr];
        if (pass == 0) mean[pt] = s / 256.f;
        else rstd[pt] = 1.0f / sqrtf(s / 256.f + eps);
      }
      __syncthreads();
    }
    const float4 g0 = *reinterpret_cast<const float4*>(g + cw + 8 * fg), g1 = *reinterpret_cast<const float4*>(g + cw + 8 * fg + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(b + cw + 8 * fg), b1 = *reinterpret_cast<const float4*>(b + cw + 8 * fg + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int pt = 0; pt < 4; pt++) {
      float y[8];
#pragma unroll
      for (int q = 0; q < 8; q++) y[q] = (x[pt][q] - mean[pt]) * rstd[pt] * gg[q] + bb[q];
      bf16x8 hi, lo;
      split8(y, hi, lo);
      const uint32_t o = lsw(pt * 16 + fr, wave * 4 + fg);
      *reinterpret_cast<bf16x8*>(s_hh + o) = hi;
      *reinterpret_cast<bf16x8*>(s_hl + o) = lo;
    }
    __syncthreads();
  };
  // x is only needed at the residual adds and the LayerNorms: between them it is parked in the tile's own
  // rows of S.x (nobody else reads them), which frees 32 VGPRs for the GEMM / attention phases
  auto park_x = [&]() {
#pragma unroll
    for (int pt = 0; pt < 4; pt++) {
      const uint32_t tok = pt * 16 + fr;
      if (tok < nt) {
        float* xp = S.x + (uint64_t)(t0 + tok) * 256 + cw + 8 * fg;
        *reinterpret_cast<float4*>(xp) = make_float4(x[pt][0], x[pt][1], x[pt][2], x[pt][3]);
        *reinterpret_cast<float4*>(xp + 4) = make_float4(x[pt][4], x[pt][5], x[pt][6], x[pt][7]);
      }
    }
  };
  auto fetch_x = [&]() {
#pragma unroll
    for (int pt = 0; pt < 4; pt++) {
      const uint32_t tok = pt * 16 + fr;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (tok < nt) {
        const float* xp = S.x + (uint64_t)(t0 + tok) * 256 + cw + 8 * fg;
        a = *reinterpret_cast<const float4*>(xp);
        b = *reinterpret_cast<const float4*>(xp + 4);
      }
      x[pt][0] = a.x; x[pt][1] = a.y; x[pt][2] = a.z; x[pt][3] = a.w;
      x[pt][4] = b.x; x[pt][5] = b.y; x[pt][6] = b.z; x[pt][7] = b.w;
    }
  };
  auto zero = [](f32x4 (&a)[4][2]) {
#pragma unroll
    for (int pt = 0; pt < 4; pt++)
#pragma unroll
      for (int jt = 0; jt < 2; jt++) a[pt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto bias8 = [&](const float* bias, uint32_t c, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(bias + c), b = *reinterpret_cast<const float4*>(bias + c + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  };

  const float scale = 1.0f / sqrtf(32.f);
  fetch_x();
  for (uint32_t li = 0; li < M.h.n_layers; li++) {
    const LayerW& L = M.layer[li];
    layer_norm(L.ln1_g, L.ln1_b);
    if (li) park_x();  // (first layer: S.x still holds it)
    {  // ---- attention, head = wave
      bf16x8 qh[4], ql[4], kh[4], kl[4], vh[2][2], vl[2][2];
      {
        f32x4 a[4][2];
        float bq[8];
        zero(a);
        tile_gemm<false>(L.qkv, cw, 0, s_hh, s_hl, fr, fg, a);
        bias8(L.qkv.bias, cw + 8 * fg, bq);
#pragma unroll
        for (int pt = 0; pt < 4; pt++) {
          float v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = (a[pt][q >> 2][q & 3] + bq[q]) * scale;
          split8(v, qh[pt], ql[pt]);
        }
        zero(a);
        tile_gemm<false>(L.qkv, 256 + cw, 0, s_hh, s_hl, fr, fg, a);
        bias8(L.qkv.bias, 256 + cw + 8 * fg, bq);
#pragma unroll
        for (int pt = 0; pt < 4; pt++) {
          float v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = a[pt][q >> 2][q & 3] + bq[q];
          split8(v, kh[pt], kl[pt]);
        }
        zero(a);
        tile_gemm<true>(L.qkv, 512 + cw, 0, s_hh, s_hl, fr, fg, a);
        // lane = channel 512 + cw + 8 (fr>>2) + 4 ct + (fr&3), tokens 16 pt + 4 fg + r
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
          const float bv = L.qkv.bias[512 + cw + 8 * (fr >> 2) + 4 * ct + (fr & 3)];
#pragma unroll
          for (int kk = 0; kk < 2; kk++) {  // k-step of 32 tokens: slots e < 4 from token tile 2kk, e >= 4 from 2kk + 1
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = a[2 * kk + (e >> 2)][ct][e & 3] + bv;
            split8(v, vh[ct][kk], vl[ct][kk]);
          }
        }
      }
      uint32_t wj[4][4];
#pragma unroll
      for (int pj = 0; pj < 4; pj++)
#pragma unroll
        for (int r = 0; r < 4; r++) wj[pj][r] = s_win[pj * 16 + 4 * fg + r];
#pragma unroll
      for (int pi = 0; pi < 4; pi++) {
        const uint32_t wi = s_win[pi * 16 + fr];
        f32x4 st[4];  // S^T: lane = query pi*16 + fr, keys pj*16 + 4 fg + r
        float m = -INFINITY;
#pragma unroll
        for (int pj = 0; pj < 4; pj++) {
          st[pj] = f32x4{0.f, 0.f, 0.f, 0.f};
          st[pj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl[pj], qh[pi], st[pj], 0, 0, 0);
          st[pj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh[pj], ql[pi], st[pj], 0, 0, 0);
          st[pj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh[pj], qh[pi], st[pj], 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            st[pj][r] = wj[pj][r] == wi ? st[pj][r] : -INFINITY;
            m = fmaxf(m, st[pj][r]);
          }
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int pj = 0; pj < 4; pj++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float pexp = __expf(st[pj][r] - m);  // masked keys: exp(-inf) = 0; a query always sees itself
            st[pj][r] = pexp;
            l += pexp;
          }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = st[2 * kk + (e >> 2)][e & 3];
          bf16x8 ph, pl;
          split8(v, ph, pl);
#pragma unroll
          for (int ct = 0; ct < 2; ct++) {
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl[ct][kk], ph, o[ct], 0, 0, 0);
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh[ct][kk], pl, o[ct], 0, 0, 0);
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh[ct][kk], ph, o[ct], 0, 0, 0);
          }
        }
        // O^T: lane = query pi*16 + fr, channels cw + 8 fg + 4 ct + r
        const float inv = 1.0f / l;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = o[e >> 2][e & 3] * inv;
        bf16x8 hi, lo;
        split8(v, hi, lo);
        const uint32_t oo = lsw(pi * 16 + fr, wave * 4 + fg);
        *reinterpret_cast<bf16x8*>(s_ah + oo) = hi;
        *reinterpret_cast<bf16x8*>(s_al + oo) = lo;
      }
    }
    __syncthreads();
    {  // ---- output projection + residual
      f32x4 a[4][2];
      float bp[8];
      zero(a);
      tile_gemm<false>(L.proj, cw, 0, s_ah, s_al, fr, fg, a);
      bias8(L.proj.bias, cw + 8 * fg, bp);
      fetch_x();
#pragma unroll
      for (int pt = 0; pt < 4; pt++)
#pragma unroll
        for (int q = 0; q < 8; q++) x[pt][q] += a[pt][q >> 2][q & 3] + bp[q];
    }
    layer_norm(L.ln2_g, L.ln2_b);  // its barriers also fence the reuse of s_ah / s_al below
    park_x();
    {  // ---- feed-forward, 256 hidden channels at a time
      f32x4 a2[4][2];
      zero(a2);
      for (uint32_t c = 0; c < M.h.d_ff; c += 256) {
        f32x4 a1[4][2];
        float b1[8];
        zero(a1);
        tile_gemm<false>(L.ff1, c + cw, 0, s_hh, s_hl, fr, fg, a1);
        bias8(L.ff1.bias, c + cw + 8 * fg, b1);
#pragma unroll
        for (int pt = 0; pt < 4; pt++) {
          float v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = fmaxf(a1[pt][q >> 2][q & 3] + b1[q], 0.f);
          bf16x8 hi, lo;
          split8(v, hi, lo);
          const uint32_t oo = lsw(pt * 16 + fr, wave * 4 + fg);
          *reinterpret_cast<bf16x8*>(s_ah + oo) = hi;
          *reinterpret_cast<bf16x8*>(s_al + oo) = lo;
        }
        __syncthreads();
        tile_gemm<false>(L.ff2, cw, c, s_ah, s_al, fr, fg, a2);
        __syncthreads();
      }
      float b2[8];
      bias8(L.ff2.bias, cw + 8 * fg, b2);
      fetch_x();
#pragma unroll
      for (int pt = 0; pt < 4; pt++)
#pragma unroll
        for (int q = 0; q < 8; q++) x[pt][q] += a2[pt][q >> 2][q & 3] + b2[q];
    }
  }
  layer_norm(M.lnf_g, M.lnf_b);
  // ---- heads: 16 output channels (0 info, 1..5 bases); wave w < 4 takes token tile w
  if (wave < 4) {
    const uint32_t pt = wave;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    const Weight& W = M.heads;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      const bf16x8 wh = *reinterpret_cast<const bf16x8*>(W.hi + (uint64_t)fr * 256 + ks * 32 + fg * 8);
      const bf16x8 wl = *reinterpret_cast<const bf16x8*>(W.lo + (uint64_t)fr * 256 + ks * 32 + fg * 8);
      const uint32_t o = lsw(pt * 16 + fr, ks * 4 + fg);
      const bf16x8 xh = *reinterpret_cast<const bf16x8*>(s_hh + o);
      const bf16x8 xl = *reinterpret_cast<const bf16x8*>(s_hl + o);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, a, 0, 0, 0);
    }
    // lane = token pt*16 + fr, channels 4 fg + r
    const uint32_t tok = pt * 16 + fr;
    if (tok < nt) {
      const uint32_t n = t0 + tok, b = S.tok_win[n];
      const uint64_t o = B.out_off[b] + (n - B.tok_off[b]);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t ch = 4 * fg + r;
        const float v = a[r] + W.bias[ch];
        if (ch == 0) B.out_info[o] = v;
        else if (ch < 6) B.out_base[o * 5 + (ch - 1)] = v;
      }
    }
  }
}

// The front of the model in bf16x3 for ANY conv stack of the family: token table, embedding + conv1 + conv2, the projection over the 31 rows, the position
// term -> S.x (f32).  Used by launch_model_s below and (round 6) by launch_model_h when a model has the f16 stack's encoder shapes but another conv stack.
void launch_front_generic(const ModelDev& M, const BatchDev& B, const ModelScratch& S, hipStream_t st, KernelTimer* tm, uint32_t n_cu, FrontEndPlan* ran) {
  const uint32_t N = B.n_tok;
  const ModelHyper& h = M.h;
  const uint32_t D = h.d_model;
  KT_BEGIN(tm, "build_tokens", st);
  hipLaunchKernelGGL(k_build_tokens, dim3(B.n_win), dim3(64), 0, st, B, S);
  KT_END(tm, st);
  const uint32_t P = 4 * (h.kw / 2) + 1;
  if (ran) *ran = FrontEndPlan{false, 0, 0, 0, 0};
  if (h.c2 == FC2 && h.c1 == 64 && h.kw == 3) {
    const uint32_t n_tiles = (N * HERRO_ROWS + CW_TP - 1) / CW_TP;
    KT_BEGIN(tm, "conv_fused", st);
    const uint32_t grid = conv_w_grid(n_tiles, std::max(n_cu, 1u));   // a stride loop over the tiles, two workgroups per compute unit
    hipLaunchKernelGGL(k_conv_w, dim3(grid), dim3(256), CW_SHM, st, M, B, S, N * HERRO_ROWS, n_tiles);
    KT_END(tm, st);
    if (ran) *ran = FrontEndPlan{false, 0, 0, grid, n_tiles};
  } else {
    const size_t shm = (size_t)(h.kw * 12 * h.c1 + h.kw * h.c1 + h.c1 + HERRO_ROWS * P) * 4 + (size_t)HERRO_ROWS * P * 4;
    KT_BEGIN(tm, "patch_conv1", st);
    hipLaunchKernelGGL(k_patch_conv1_s, dim3((N + TOKB - 1) / TOKB), dim3(256), shm, st, M, B, S, N);
    KT_END(tm, st);
    KT_BEGIN(tm, "conv2_gemm", st);
    gemm_s(S.y1_hi, S.y1_lo, h.kw * h.c1, M.conv2, nullptr, S.y2_hi, S.y2_lo, h.c2, nullptr, N * HERRO_ROWS, 1, st);
    KT_END(tm, st);
  }
  KT_BEGIN(tm, "fc_gemm", st);
  gemm_s(S.y2_hi, S.y2_lo, HERRO_ROWS * h.c2, M.fc, S.x, nullptr, nullptr, D, nullptr, N, 0, st);
  KT_END(tm, st);
  KT_BEGIN(tm, "add_pe", st);
  if (M.pe_kind != 2) {
    const uint64_t tot = (uint64_t)N * (D / 2);
    hipLaunchKernelGGL(k_add_pe, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, st, M, S, N);
  }
  KT_END(tm, st);
}

static void launch_model_s(const ModelDev& M, const BatchDev& B, const ModelScratch& S, bool fused, hipStream_t st, KernelTimer* tm, uint32_t n_cu, FrontEndPlan* ran) {
  const uint32_t N = B.n_tok;
  const ModelHyper& h = M.h;
  const uint32_t D = h.d_model;
  launch_front_generic(M, B, S, st, tm, n_cu, ran);
  if (fused && B.n_tiles && D == 256 && h.n_heads == 8 && h.d_ff % 256 == 0 && model_default_variant(M)) {
    opt_in_dynamic_lds(reinterpret_cast<const void*>(k_layers), LAYERS_SHM);
    KT_BEGIN(tm, "layers_fused", st);
    hipLaunchKernelGGL(k_layers, dim3(B.n_tiles), dim3(512), LAYERS_SHM, st, M, B, S);
    KT_END(tm, st);
    return;
  }
  // Layer by layer: every variant of the family (round 6).  Pre-LN: x += f(LN(x)); Post-LN: x = LN(x + f(x)) — the LayerNorm output is then the residual
  // stream itself (written back as f32 next to the planes the next GEMM reads), and the first layer's QKV reads the split of x as it is.
  const dim3 ln_grid((N + 3) / 4);
  const bool pre = M.norm_first != 0;
  const int ff_act = 1 + (int)M.act;   // apply_act: 1 ReLU, 2 GELU (erf), 3 GELU (tanh)
  const uint32_t dh = D / h.n_heads;
  auto ln = [&](const float* g, const float* b, float* xo) {
    KT_BEGIN(tm, "layernorm", st);
    hipLaunchKernelGGL(k_layernorm_s, ln_grid, dim3(256), 0, st, S.x, S.h_hi, S.h_lo, g, b, N, D, h.ln_eps, xo);
    KT_END(tm, st);
  };
  if (!pre) ln(nullptr, nullptr, nullptr);   // planes of x
  for (uint32_t li = 0; li < h.n_layers; li++) {
    const LayerW& L = M.layer[li];
    if (pre) ln(L.ln1_g, L.ln1_b, nullptr);
    KT_BEGIN(tm, "qkv_gemm", st);
    gemm_s(S.h_hi, S.h_lo, D, L.qkv, S.qkv, nullptr, nullptr, 3 * D, nullptr, N, 0, st);
    KT_END(tm, st);
    KT_BEGIN(tm, "attention", st);
    {
      const dim3 grid(B.n_win, std::max(1u, std::min((B.max_win_tok + 15) / 16, 64u)));
      if (dh == 64) hipLaunchKernelGGL(k_attention_s<64>, grid, dim3(16 * h.n_heads), (size_t)2 * KC * D * 4, st, B, S, D);
      else hipLaunchKernelGGL(k_attention_s<32>, grid, dim3(16 * h.n_heads), (size_t)2 * KC * D * 4, st, B, S, D);
    }
    KT_END(tm, st);
    KT_BEGIN(tm, "proj_gemm", st);
    gemm_s(S.att_hi, S.att_lo, D, L.proj, S.x, nullptr, nullptr, D, S.x, N, 0, st);
    KT_END(tm, st);
    if (pre) ln(L.ln2_g, L.ln2_b, nullptr); else ln(L.ln1_g, L.ln1_b, S.x);
    KT_BEGIN(tm, "ff1_gemm", st);
    gemm_s(S.h_hi, S.h_lo, D, L.ff1, nullptr, S.ff_hi, S.ff_lo, h.d_ff, nullptr, N, ff_act, st);
    KT_END(tm, st);
    KT_BEGIN(tm, "ff2_gemm", st);
    gemm_s(S.ff_hi, S.ff_lo, h.d_ff, L.ff2, S.x, nullptr, nullptr, D, S.x, N, 0, st);
    KT_END(tm, st);
    if (!pre) ln(L.ln2_g, L.ln2_b, S.x);
  }
  if (M.final_norm) ln(M.lnf_g, M.lnf_b, nullptr);
  else if (pre) ln(nullptr, nullptr, nullptr);   // (Post-LN without a final norm: the planes of the last LayerNorm are what the heads read)
  KT_BEGIN(tm, "heads_gemm", st);
  gemm_s(S.h_hi, S.h_lo, D, M.heads, S.logits, nullptr, nullptr, 16, nullptr, N, 0, st);
  KT_END(tm, st);
  KT_BEGIN(tm, "scatter_logits", st);
  hipLaunchKernelGGL(k_scatter_logits, dim3(B.n_win), dim3(64), 0, st, B, S);
  KT_END(tm, st);
}

void launch_model(const ModelDev& M, const BatchDev& B, const ModelScratch& S, int precision,
                  hipStream_t st, KernelTimer* tm, uint32_t n_cu, FrontEndPlan* ran) {
  const uint32_t N = B.n_tok;
  if (N == 0) return;
  if (ran) *ran = FrontEndPlan{false, 0, 0, 0, 0};   // (the kernels below take no grid from n_cu: nothing to report)
  if (precision == 1 || precision == 3) {  // 3: bf16x3, layer by layer (the fused stack's fallback, selectable for A/B)
    launch_model_s(M, B, S, precision == 1, st, tm, n_cu, ran);
    return;
  }
  const ModelHyper& h = M.h;
  const uint32_t D = h.d_model;
  KT_BEGIN(tm, "build_tokens", st);
  hipLaunchKernelGGL(k_build_tokens, dim3(B.n_win), dim3(64), 0, st, B, S);
  KT_END(tm, st);

  const uint32_t P = 4 * (h.kw / 2) + 1;
  const size_t shm = (size_t)(h.kw * 12 * h.c1 + h.kw * h.c1 + h.c1 + HERRO_ROWS * P) * 4 + (size_t)HERRO_ROWS * P * 4;
  KT_BEGIN(tm, "patch_conv1", st);
  hipLaunchKernelGGL(k_patch_conv1, dim3(N), dim3(256), shm, st, M, B, S);
  KT_END(tm, st);

  KT_BEGIN(tm, "conv2_gemm", st);
  gemm(S.y1, h.kw * h.c1, M.conv2, S.y2, h.c2, nullptr, N * HERRO_ROWS, 1, precision, st);
  KT_END(tm, st);
  KT_BEGIN(tm, "fc_gemm", st);
  gemm(S.y2, HERRO_ROWS * h.c2, M.fc, S.x, D, nullptr, N, 0, precision, st);
  KT_END(tm, st);
  KT_BEGIN(tm, "add_pe", st);
  if (M.pe_kind != 2) {
    const uint64_t tot = (uint64_t)N * (D / 2);
    hipLaunchKernelGGL(k_add_pe, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, st, M, S, N);
  }
  KT_END(tm, st);

  const dim3 ln_grid((N + 3) / 4);
  const bool pre = M.norm_first != 0;
  const int ff_act = 1 + (int)M.act;
  const uint32_t dh = D / h.n_heads;
  auto ln = [&](const float* x, float* y, const float* g, const float* b) {
    KT_BEGIN(tm, "layernorm", st);
    hipLaunchKernelGGL(k_layernorm, ln_grid, dim3(256), 0, st, x, y, g, b, N, D, h.ln_eps);
    KT_END(tm, st);
  };
  for (uint32_t li = 0; li < h.n_layers; li++) {
    const LayerW& L = M.layer[li];
    if (pre) ln(S.x, S.hbuf, L.ln1_g, L.ln1_b);
    KT_BEGIN(tm, "qkv_gemm", st);
    gemm(pre ? S.hbuf : S.x, D, L.qkv, S.qkv, 3 * D, nullptr, N, 0, precision, st);
    KT_END(tm, st);
    KT_BEGIN(tm, "attention", st);
    if (dh == 64) hipLaunchKernelGGL(k_attention<64>, dim3(B.n_win, h.n_heads), dim3(64), 0, st, B, S, D);
    else hipLaunchKernelGGL(k_attention<32>, dim3(B.n_win, h.n_heads), dim3(64), 0, st, B, S, D);
    KT_END(tm, st);
    KT_BEGIN(tm, "proj_gemm", st);
    gemm(S.att, D, L.proj, S.x, D, S.x, N, 0, precision, st);
    KT_END(tm, st);
    if (pre) ln(S.x, S.hbuf, L.ln2_g, L.ln2_b); else ln(S.x, S.x, L.ln1_g, L.ln1_b);   // Post-LN: the residual stream is normalised in place
    KT_BEGIN(tm, "ff1_gemm", st);
    gemm(pre ? S.hbuf : S.x, D, L.ff1, S.ff, h.d_ff, nullptr, N, ff_act, precision, st);
    KT_END(tm, st);
    KT_BEGIN(tm, "ff2_gemm", st);
    gemm(S.ff, h.d_ff, L.ff2, S.x, D, S.x, N, 0, precision, st);
    KT_END(tm, st);
    if (!pre) ln(S.x, S.x, L.ln2_g, L.ln2_b);
  }
  if (M.final_norm) ln(S.x, S.hbuf, M.lnf_g, M.lnf_b);
  KT_BEGIN(tm, "heads_gemm", st);
  gemm(M.final_norm ? S.hbuf : S.x, D, M.heads, S.logits, 16, nullptr, N, 0, precision, st);
  KT_END(tm, st);
  KT_BEGIN(tm, "scatter_logits", st);
  hipLaunchKernelGGL(k_scatter_logits, dim3(B.n_win), dim3(64), 0, st, B, S);
  KT_END(tm, st);
}

}  // namespace herro
