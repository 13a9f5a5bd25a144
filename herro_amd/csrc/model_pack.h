// model_pack.h — the host half of herro_load_model: the flat weight file -> every byte the device will hold, and nothing of a device or a
// context.  Plain C++17 (no HIP header: a host compiler alone builds and sanitizes it).  Here are the file reader, the number formats
// (bf16, f16, OCP e4m3), the one implementation of each layout model_dev.h documents (Weight::phi, Weight::p8, ModelDev::conv1g) and
// load_host_model, which walks the tensors a model needs; model_api.hip uploads what it returns.  Test hook: herro_debug_model_pack.
#pragma once
#include <stdint.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/herro_amd.h"

namespace herro {

struct ModelHyper {  // header of the flat weight file (tools/export_weights.py)
  uint32_t magic;    // 'HRRO'
  uint32_t version;
  uint32_t rows;     // 31
  uint32_t kw;       // conv kernel width along the window axis (odd)
  uint32_t c1, c2;   // conv channels
  uint32_t d_model, n_heads, d_ff, n_layers;
  uint32_t n_tensors;
  float ln_eps;
};

// ---- the file ------------------------------------------------------------------------------------
struct HostTensor { std::vector<uint32_t> dims; std::vector<float> data; };
struct ModelFile { ModelHyper h{}; std::map<std::string, HostTensor> T; };

// header, then n_tensors x { name[32], nd <= 4, dims[4], f32 data }.  No tensor is given room before the rest of the file is known to hold it.
inline int read_model_file(const char* path, ModelFile& mf, std::string& err) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { err = std::string("cannot open model file ") + path; return HERRO_E_NO_MODEL; }
  struct stat sb;
  uint64_t left = fstat(fileno(f), &sb) == 0 && sb.st_size > 0 ? (uint64_t)sb.st_size : 0;   // bytes of the file not read yet
  auto rd = [&](void* p, uint64_t n) { if (n > left || (n && std::fread(p, n, 1, f) != 1)) return false; left -= n; return true; };
  ModelHyper& h = mf.h;
  bool ok = rd(&h, sizeof h) && h.magic == 0x4f525248u /* 'HRRO' */ && h.version == 1;
  for (uint32_t i = 0; ok && i < h.n_tensors; i++) {
    char name[32];
    uint32_t nd, dims[4];
    ok = rd(name, 32) && rd(&nd, 4) && rd(dims, 16) && nd <= 4;
    if (!ok) break;
    name[31] = 0;
    HostTensor t;
    const uint64_t room = left / 4;
    uint64_t n = 1;   // product of the dims, saturating once it is past what the file can hold (a zero dim makes it 0 wherever it stands)
    for (uint32_t d = 0; d < nd; d++) { t.dims.push_back(dims[d]); n = !dims[d] ? 0 : (n > room / dims[d] ? UINT64_MAX : n * dims[d]); }
    if (!(ok = n <= room)) break;
    t.data.resize(n);
    ok = rd(t.data.data(), n * 4);
    mf.T[name] = std::move(t);
  }
  std::fclose(f);
  if (!ok) { err = "malformed model file"; return HERRO_E_NO_MODEL; }
  return HERRO_OK;
}

// ---- number formats --------------------------------------------------------------------------------
inline uint16_t h_bf16(float f) {
  uint32_t u; std::memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float h_bf16f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f; }

// f32 -> IEEE binary16, round to nearest even (subnormals kept, overflow -> inf), and back
inline uint16_t h_f16(float f) {
  uint32_t u; std::memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u));  // inf / nan
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                     // rounds to >= 65520 -> inf
  if (a < 0x33000001u) return (uint16_t)sign;                                                  // <= 2^-25 -> 0 (ties to even)
  const int32_t e = (int32_t)(a >> 23) - 127;
  uint32_t m = (a & 0x7fffffu) | 0x800000u;   // 24-bit significand
  int shift;                                  // bits dropped from m
  uint32_t base;
  if (e >= -14) { shift = 13; base = (uint32_t)(e + 15) << 10; m &= 0x7fffffu; }   // normal: keep 10 fraction bits
  else { shift = 13 + (-14 - e); base = 0; }                                        // subnormal: value = m * 2^(e-23), unit 2^-24
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1u))) q++;
  return (uint16_t)(sign | (base + q));       // a carry out of the fraction bumps the exponent, as it must
}
inline float h_f16f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  float f;
  if (e == 0) f = std::ldexp((float)m, -24);
  else if (e == 31) f = m ? NAN : INFINITY;
  else f = std::ldexp((float)(m | 0x400u), (int)e - 25);
  uint32_t u; std::memcpy(&u, &f, 4); u |= sign; std::memcpy(&f, &u, 4);
  return f;
}

// f32 -> OCP e4m3 (e4m3fn: bias 7, 3 fraction bits, subnormals in units of 2^-9, largest finite 448 = 0x7e, no infinities), round to nearest even,
// SATURATING (the weights of precision 6 are scaled below 448 first; the device's own v_cvt_pk_fp8_f32 turns >= 480 into NaN).  Values the
// device conversion produced for the same inputs: tools/probes/mx_probe.hip (1 -> 0x38, 0.1 -> 0x1d, 3.3 -> 0x45, 0.0176 -> 0x09, 2^-9 -> 0x01, 2^-10 -> 0).
inline uint8_t f32_to_e4m3(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80u : 0u;
  const float a = std::fabs(f);
  if (!(a == a)) return (uint8_t)(sign | 0x7fu);           // NaN
  if (a >= 448.f) return (uint8_t)(sign | 0x7eu);
  if (a < std::ldexp(1.f, -6)) return (uint8_t)(sign | (uint8_t)std::nearbyint(std::ldexp(a, 9)));   // subnormal (8 -> 0x08 = the smallest normal, as it must)
  int ex;
  const float m = std::frexp(a, &ex);                      // a = m * 2^ex, m in [0.5, 1)
  int q = (int)std::nearbyint(std::ldexp(m, 4)) - 8;        // fraction of 1.fff in eighths, ties to even
  int e = ex - 1 + 7;
  if (q == 8) { q = 0; e++; }
  const int code = (e << 3) | q;
  return (uint8_t)(sign | (uint8_t)std::min(code, 0x7e));
}

// w ~= hi + lo in a 16-bit format: hi = the rounded weight, lo = the rounded remainder
struct Split16 { std::vector<uint16_t> hi, lo; };
template <uint16_t (*ENC)(float), float (*DEC)(uint16_t)>
Split16 split16(const float* w, size_t n) {
  Split16 s{std::vector<uint16_t>(n), std::vector<uint16_t>(n)};
  for (size_t i = 0; i < n; i++) { s.hi[i] = ENC(w[i]); s.lo[i] = ENC(w[i] - DEC(s.hi[i])); }
  return s;
}
inline Split16 split_bf16(const float* w, size_t n) { return split16<h_bf16, h_bf16f>(w, n); }
inline Split16 split_f16(const float* w, size_t n) { return split16<h_f16, h_f16f>(w, n); }

// ---- MFMA fragment order (model_dev.h: Weight::phi, Weight::p8) ------------------------------------------------------
// the row of src ([N][K] row-major) that lane 16 fg + fr of B-fragment jt of 32-column block n32 holds
inline size_t frag_row(uint32_t n32, uint32_t jt, uint32_t lane) { const uint32_t fr = lane & 15; return (size_t)n32 * 32 + 8 * (fr >> 2) + 4 * jt + (fr & 3); }

// Weight::phi: 8 consecutive k per lane, 32 per step.  K, N multiples of 32.
inline std::vector<uint16_t> pack_frag16(const uint16_t* src, uint32_t K, uint32_t N) {
  std::vector<uint16_t> out((size_t)K * N);
  const uint32_t nks = K / 32;
  uint16_t* dst = out.data();
  for (uint32_t n32 = 0; n32 < N / 32; n32++)
    for (uint32_t jt = 0; jt < 2; jt++)
      for (uint32_t ks = 0; ks < nks; ks++)
        for (uint32_t lane = 0; lane < 64; lane++, dst += 8)
          std::memcpy(dst, src + frag_row(n32, jt, lane) * K + ks * 32 + (lane >> 4) * 8, 16);
  return out;
}

// Weight::p8: OCP e4m3 of W * 2^sw, 16 consecutive k per lane and half, 128 per step; sw = the largest power of two that keeps
// max |W| * 2^sw <= 448, within +-32 (0 for an all-zero or non-finite maximum); s8 = 127 - sw, the E8M0 byte that undoes it.  K % 128 == 0, N % 32 == 0.
inline std::vector<uint8_t> pack_frag8(const float* w, uint32_t K, uint32_t N, uint32_t& s8) {
  float wmax = 0.f;
  for (size_t i = 0; i < (size_t)K * N; i++) wmax = std::max(wmax, std::fabs(w[i]));
  int sw = 0;
  if (wmax > 0.f && std::isfinite(wmax)) { int ex; (void)std::frexp(448.0 / (double)wmax, &ex); sw = std::max(-32, std::min(32, ex - 1)); }
  s8 = (uint32_t)(127 - sw);
  std::vector<uint8_t> out((size_t)K * N);
  const uint32_t ns = K / 128;
  const float mul = std::ldexp(1.0f, sw);
  uint8_t* dst = out.data();
  for (uint32_t n32 = 0; n32 < N / 32; n32++)
    for (uint32_t jt = 0; jt < 2; jt++)
      for (uint32_t st = 0; st < ns; st++)
        for (uint32_t hf = 0; hf < 2; hf++)
          for (uint32_t lane = 0; lane < 64; lane++, dst += 16) {
            const float* src = w + frag_row(n32, jt, lane) * K + st * 128 + (lane >> 4) * 32 + hf * 16;
            for (uint32_t j = 0; j < 16; j++) dst[j] = f32_to_e4m3(src[j] * mul);
          }
  return out;
}

// conv1 as a GEMM (k_conv_m; kw 3, c1 64): W1g[c][tap * 32 + slot] in f16, [64][96].  Slots of a tap: 0..11 the table row of each token (hi),
// 13 and 14 the quality weight (hi), 15 the bias (hi, tap 0 only), 16..27 / 29 / 31 their remainders (lo); the others 0.
inline std::vector<uint16_t> conv1_gemm_rows(const float* t1, const float* wq1, const float* b1) {
  const uint32_t K = 96, N = 64;
  std::vector<uint16_t> g((size_t)N * K, 0);
  auto hl = [](float v, uint16_t& hi, uint16_t& lo) { hi = h_f16(v); lo = h_f16(v - h_f16f(hi)); };
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t tp = 0; tp < 3; tp++) {
      uint16_t* row = g.data() + (size_t)c * K + tp * 32;
      for (uint32_t tok = 0; tok < 12; tok++) hl(t1[((size_t)tp * 12 + tok) * N + c], row[tok], row[16 + tok]);
      uint16_t qh, ql;
      hl(wq1[(size_t)tp * N + c], qh, ql);
      row[13] = qh; row[14] = qh; row[29] = ql;
      if (tp == 0) hl(b1[c], row[15], row[31]);
    }
  return g;
}

// ---- a model on the host ----------------------------------------------------------------------------
// One device array to be: borrowed from the file's tensors (f32) or owned (the converted and shuffled copies).
struct Blob {
  const void* p = nullptr;
  size_t bytes = 0;
  std::vector<uint16_t> u16;
  std::vector<uint8_t> u8;
};
// ModelDev (model_dev.h) with an index into HostModel::blobs where that holds a device pointer (-1: null)
enum WForm { W_F32, W_HI, W_LO, W_PHI, W_PLO, W_H16, W_L16, W_PH16, W_P8, W_BIAS, W_FORMS };
struct HostWeight {
  uint32_t K = 0, N = 0, s8 = 127;
  int blob[W_FORMS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
};
struct HostLayer {
  int ln1_g = -1, ln1_b = -1, ln2_g = -1, ln2_b = -1;
  HostWeight qkv, proj, ff1, ff2;
};
struct HostModel {
  ModelFile file;             // (the f32 blobs point into it)
  std::vector<Blob> blobs;
  float wmax = 0.f;           // largest |weight| of the GEMM weights
  int t1 = -1, wq1 = -1, b1 = -1, pe_div = -1, lnf_g = -1, lnf_b = -1, pe_learned = -1;
  HostWeight conv1g, conv2, fc, heads;
  HostLayer layer[16];
  uint32_t act = 0, norm_first = 1, pe_kind = 0, final_norm = 1, pe_learned_rows = 0;

  int borrow(const std::vector<float>& v) { Blob b; b.p = v.data(); b.bytes = v.size() * 4; blobs.push_back(std::move(b)); return (int)blobs.size() - 1; }
  int own(std::vector<uint16_t>&& v) { Blob b; b.u16 = std::move(v); b.p = b.u16.data(); b.bytes = b.u16.size() * 2; blobs.push_back(std::move(b)); return (int)blobs.size() - 1; }
  int own(std::vector<uint8_t>&& v) { Blob b; b.u8 = std::move(v); b.p = b.u8.data(); b.bytes = b.u8.size(); blobs.push_back(std::move(b)); return (int)blobs.size() - 1; }
};

// every form of one [N][K] weight the kernels read (model_dev.h: Weight)
inline void pack_weight(HostModel& hm, HostWeight& w, const std::vector<float>& wt) {
  const uint32_t K = w.K, N = w.N;
  for (float x : wt) hm.wmax = std::max(hm.wmax, std::fabs(x));
  w.blob[W_F32] = hm.borrow(wt);
  const bool frag = N % 32 == 0 && K % 32 == 0;   // fragment-ordered copies for the kernels that stream weights into registers
  auto plane = [&](WForm f) { return (const uint16_t*)hm.blobs[w.blob[f]].p; };   // (a blob's bytes stay where they are when the list grows)
  Split16 b = split_bf16(wt.data(), wt.size());
  w.blob[W_HI] = hm.own(std::move(b.hi)); w.blob[W_LO] = hm.own(std::move(b.lo));
  if (frag) { w.blob[W_PHI] = hm.own(pack_frag16(plane(W_HI), K, N)); w.blob[W_PLO] = hm.own(pack_frag16(plane(W_LO), K, N)); }
  Split16 h = split_f16(wt.data(), wt.size());   // f16 forms (precision 4 .. 8, model_h.hip)
  w.blob[W_H16] = hm.own(std::move(h.hi)); w.blob[W_L16] = hm.own(std::move(h.lo));
  if (frag) w.blob[W_PH16] = hm.own(pack_frag16(plane(W_H16), K, N));
  if (N % 32 == 0 && K % 128 == 0) w.blob[W_P8] = hm.own(pack_frag8(wt.data(), K, N, w.s8));   // the remainder term of precision 6
}

// path -> the complete host form of the model, or the code and text herro_load_model fails with
inline int load_host_model(const char* path, HostModel& hm, std::string& err) {
  if (const int rc = read_model_file(path, hm.file, err)) return rc;
  const ModelHyper& h = hm.file.h;
  const std::map<std::string, HostTensor>& T = hm.file.T;
  if (h.rows != HERRO_ROWS || h.n_layers > 16 || (h.kw & 1) == 0 || h.d_model % 64 || h.n_heads == 0 || h.d_model % h.n_heads || (h.d_model / h.n_heads != 32 && h.d_model / h.n_heads != 64) || h.n_heads > 32 ||
      (h.kw * h.c1) % 32 || (h.rows * h.c2) % 32 || h.d_ff % 32 || h.c2 % 16) {
    err = "unsupported model hyper-parameters";
    return HERRO_E_UNSUPPORTED;
  }
  bool missing = false;
  auto get = [&](const std::string& n, size_t expect) -> const std::vector<float>* {
    auto it = T.find(n);
    if (it == T.end() || it->second.data.size() != expect) { missing = true; err = "model tensor missing/mis-sized: " + n; return nullptr; }
    return &it->second.data;
  };
  auto vec = [&](const std::string& n, size_t expect) {
    const std::vector<float>* v = get(n, expect);
    return v && !missing ? hm.borrow(*v) : -1;
  };
  auto weight = [&](const std::string& n, uint32_t K, uint32_t N) {
    HostWeight w;
    w.K = K; w.N = N;
    const std::vector<float>* wt = get(n + ".wt", (size_t)K * N);
    if (missing) return w;
    pack_weight(hm, w, *wt);
    w.blob[W_BIAS] = vec(n + ".b", N);
    return w;
  };
  const uint32_t D = h.d_model;
  hm.t1 = vec("t1", (size_t)h.kw * 12 * h.c1);
  hm.wq1 = vec("wq1", (size_t)h.kw * h.c1);
  hm.b1 = vec("b1", h.c1);
  if (!missing && h.kw == 3 && h.c1 == 64) {
    hm.conv1g.K = 96; hm.conv1g.N = 64;
    hm.conv1g.blob[W_PH16] = hm.own(pack_frag16(conv1_gemm_rows(T.at("t1").data.data(), T.at("wq1").data.data(), T.at("b1").data.data()).data(), 96, 64));
  }
  hm.conv2 = weight("conv2", h.kw * h.c1, h.c2);
  hm.fc = weight("fc", h.rows * h.c2, D);
  hm.pe_div = vec("pe_div", D / 2);
  for (uint32_t l = 0; l < h.n_layers && !missing; l++) {
    const std::string p = "L" + std::to_string(l) + ".";
    HostLayer& y = hm.layer[l];
    y.ln1_g = vec(p + "ln1.g", D); y.ln1_b = vec(p + "ln1.b", D);
    y.ln2_g = vec(p + "ln2.g", D); y.ln2_b = vec(p + "ln2.b", D);
    y.qkv = weight(p + "qkv", D, 3 * D);
    y.proj = weight(p + "proj", D, D);
    y.ff1 = weight(p + "ff1", D, h.d_ff);
    y.ff2 = weight(p + "ff2", h.d_ff, D);
  }
  if (auto it = T.find("cfg"); it != T.end()) {   // a variant of the family (absent: the defaults)
    const std::vector<float>& c = it->second.data;
    if (c.size() < 4 || c[0] < 0 || c[0] > 2 || c[1] < 0 || c[1] > 1 || c[2] < 0 || c[2] > 2 || c[3] < 0 || c[3] > 1) { err = "model file: cfg tensor not understood"; return HERRO_E_UNSUPPORTED; }
    hm.act = (uint32_t)c[0]; hm.norm_first = (uint32_t)c[1]; hm.pe_kind = (uint32_t)c[2]; hm.final_norm = (uint32_t)c[3];
  }
  if (hm.pe_kind == 1) {
    auto it = T.find("pe_table");
    if (it == T.end() || it->second.dims.size() != 2 || it->second.dims[1] != D || it->second.dims[0] == 0) { err = "model file: learned position table missing / mis-shaped"; return HERRO_E_NO_MODEL; }
    hm.pe_learned = hm.borrow(it->second.data);
    hm.pe_learned_rows = it->second.dims[0];
  }
  if (hm.final_norm) { hm.lnf_g = vec("lnf.g", D); hm.lnf_b = vec("lnf.b", D); }
  hm.heads = weight("heads", D, 16);
  return missing ? HERRO_E_NO_MODEL : HERRO_OK;
}

}  // namespace herro
