// The MobileNet backbone as one C call per direction (include/ttk.h, "The MobileNet backbone as ONE call per direction").
// HOST code only: this file launches no kernel of its own, it issues the public ttk_* entry points in the order and with the arguments
// of the Python host in its product configuration (trackertraincode/backbones/mobilenet_v1.py _forward_impl / _backward_impl and
// _mobilenet_bc.py forward_impl / backward_impl).  tests/test_native_sequence_gpu.py holds the two to the same launch list and to
// bitwise equal results.
//
// One emitter per direction and precision serves three uses: a dry run that only counts and names the calls (plan_init's validation,
// ttk_mobilenet_describe) and the real run.  TTK_SEQ_CALL evaluates its arguments only in a real run.
#include <string.h>

#include "ttk_common.h"

namespace {
using namespace ttk;

constexpr int kMaxBlocks = TTK_MOBILENET_MAX_BLOCKS;
constexpr int kEs[2] = {4, 2};  // bytes per activation element: fp32, bf16-compute

inline bool tuned_c(int c) { return c >= 32 && c <= 1024 && (c & (c - 1)) == 0; }
inline bool anyc_c(int c) { return c >= 8 && c <= 2048 && c % 8 == 0; }
inline uint64_t align256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
inline uint64_t pad64(uint64_t n) { return (n + 63) / 64 * 64; }

// the reference's block table (backbones/mobilenet_v1.py:128-140): the only one the bf16-compute kernels are built for
constexpr int kRefCin[13] = {32, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024};
constexpr int kRefCout[13] = {64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024};
constexpr int kRefStride[13] = {1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1};

struct Blk {
  int h, w, ho, wo, cin, cout, stride;
  bool skip, head, store_in, blur, t_in, t_pw, t_out;
  int64_t M;  // output pixels
};
struct Geo {
  int n, Ho, Wo, hl, wl;  // stem output, last map
  bool bc;
  Blk b[kMaxBlocks];
};

void geometry(const ttk_mobilenet_plan& p, Geo& g) {
  g.n = p.nblocks;
  g.bc = p.precision == TTK_MOBILENET_BF16_COMPUTE;
  g.Ho = (p.H + 1) / 2;
  g.Wo = (p.W + 1) / 2;
  int h = g.Ho, w = g.Wo;
  bool prev_skip = false;
  for (int k = 0; k < p.nblocks; ++k) {
    Blk& b = g.b[k];
    b.h = h, b.w = w, b.cin = p.cin[k], b.cout = p.cout[k], b.stride = p.stride[k];
    b.ho = (h - 1) / b.stride + 1, b.wo = (w - 1) / b.stride + 1;
    b.M = (int64_t)p.B * b.ho * b.wo;
    b.skip = b.stride == 1 && b.cin == b.cout;
    b.t_in = tuned_c(b.cin), b.t_out = tuned_c(b.cout), b.t_pw = b.t_in && b.t_out;
    // the raw residual operand: the first block of a chain of residual blocks, dw3_1 and dw4_1 of the table, on the tuned kernels
    b.head = !g.bc && b.skip && !prev_skip && b.t_in && (k == 2 || k == 4);
    b.store_in = b.skip && !b.head;
    b.blur = p.blur[k] != 0;
    prev_skip = b.skip;
    h = b.ho, w = b.wo;
  }
  g.hl = h, g.wl = w;
}

uint64_t plan_check(const ttk_mobilenet_plan& p) {  // FNV-1a over the plan's inputs and its sizes
  uint64_t hsh = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { for (int i = 0; i < 8; ++i) { hsh ^= (v >> (8 * i)) & 255; hsh *= 1099511628211ull; } };
  for (int v : {p.B, p.H, p.W, p.c0, p.nblocks, p.mode, p.precision, p.deterministic}) mix((uint64_t)(int64_t)v);
  for (int k = 0; k < kMaxBlocks; ++k) mix(((uint64_t)(uint32_t)p.cin[k] << 32) | (uint32_t)p.cout[k]), mix(((uint64_t)(uint32_t)p.stride[k] << 32) | (uint32_t)p.blur[k]);
  mix(p.ws_bytes[0]), mix(p.ws_bytes[1]), mix(p.arena_floats), mix(0x74746b6d6f62696cull);
  return hsh;
}
bool plan_ok(const ttk_mobilenet_plan* p) { return p && p->nblocks >= 1 && p->nblocks <= kMaxBlocks && p->ws_bytes[0] && p->check == plan_check(*p); }

// ---- the launch sequence ------------------------------------------------------------------------------------------------------
struct Seq {
  bool dry;
  char* names;       // dry: the list of names (nullable: count only)
  size_t cap, len;   // len counts the bytes the list takes, whether they fit or not
  int count;
  bool note(const char* name) {
    ++count;
    if (dry) {
      const size_t n = strlen(name);
      if (names && len + n + 1 <= cap) { memcpy(names + len, name, n); names[len + n] = '\n'; }
      len += n + 1;
    }
    return !dry;
  }
};
#define TTK_SEQ_CALL(s, fn, ...)                       \
  do {                                                 \
    if ((s).note(#fn)) {                               \
      const int rc_ = fn(__VA_ARGS__);                 \
      if (rc_ != 0) return rc_;                        \
    }                                                  \
  } while (0)
#define TTK_SEQ_TRY(expr)            \
  do {                               \
    const int rc2_ = (expr);         \
    if (rc2_ != 0) return rc2_;      \
  } while (0)

struct Args {  // everything a real run reads; a dry run has all pointers null
  const float* x = nullptr;
  const float* const* params = nullptr;
  void* const* buffers = nullptr;
  const float* const* blur = nullptr;
  float momentum = 0.f, eps = 0.f;
  char* fws = nullptr;  // forward workspace
  char* bws = nullptr;  // backward workspace
  float* feat = nullptr;
  const float* gfeat = nullptr;
  float* arena = nullptr;
  ttk_mobilenet_ready_fn on_ready = nullptr;
  void* user = nullptr;
  ttk_stream_t stream = nullptr;
};

// elements of parameter q (stem weight, gamma, beta, then per block depthwise weight, gamma, beta, pointwise weight, gamma, beta)
size_t param_numel(const ttk_mobilenet_plan& p, int q) {
  if (q < 3) return q == 0 ? (size_t)p.c0 * 25 : (size_t)p.c0;
  const int k = (q - 3) / 6, r = (q - 3) % 6;
  return r == 0 ? (size_t)p.cin[k] * 9 : r < 3 ? (size_t)p.cin[k] : r == 3 ? (size_t)p.cin[k] * p.cout[k] : (size_t)p.cout[k];
}

// float offsets, computed once per call: BatchNorm constant block `bi` inside its arena (0 = stem, 1 + 2k = block k's depthwise, 2 + 2k = its
// pointwise) and parameter i's slice of the gradient arena
struct Offsets {
  size_t bn[1 + 2 * kMaxBlocks], grad[3 + 6 * kMaxBlocks + 1];
  explicit Offsets(const ttk_mobilenet_plan& p) {
    size_t off = 0;
    for (int i = 0; i < 1 + 2 * p.nblocks; ++i) {
      bn[i] = off;
      off += (size_t)TTK_BN_ROWS * (i == 0 ? p.c0 : (i & 1) ? p.cin[(i - 1) / 2] : p.cout[(i - 2) / 2]);
    }
    off = 0;
    for (int q = 0; q < 3 + 6 * p.nblocks; ++q) grad[q] = off, off += pad64(param_numel(p, q));
    grad[3 + 6 * p.nblocks] = off;
  }
};

struct Ctx {
  const ttk_mobilenet_plan& p;
  const Geo& g;
  const Args& a;
  Seq& s;
  const Offsets& o;
  char* buf(int which, int idx) const {
    char* base = which ? a.bws : a.fws;
    return (idx < 0 || !base) ? nullptr : base + p.buf_off[which][idx];
  }
  float* fbuf(int which, int idx) const { return reinterpret_cast<float*>(buf(which, idx)); }
  const float* P(int i) const { return a.params ? a.params[i] : nullptr; }
  float* Bf(int i) const { return a.buffers ? static_cast<float*>(a.buffers[i]) : nullptr; }
  const float* blurw(int k) const { return a.blur ? a.blur[k] : nullptr; }
  float* bn(int bi) const {
    float* base = fbuf(0, p.i_bn);
    return base ? base + o.bn[bi] : nullptr;
  }
  float* grad(int i) const { return a.arena ? a.arena + o.grad[i] : nullptr; }
};

// a stage: a raw conv output, its BatchNorm block, and the residual operand added before the ReLU (stored, or raw with its own block)
struct Stage {
  char* y = nullptr;
  float* bn = nullptr;
  char* skip = nullptr;
  float* skip_bn = nullptr;
  bool has_skip = false, raw = false;  // (the flags, not the pointers, steer the sequence: a dry run has no pointers)
};
// the stages of the network from the plan alone: index 0 = stem, 1 + 2k = block k depthwise, 2 + 2k = block k pointwise
Stage stage_of(const Ctx& c, int si) {
  Stage st;
  const auto& p = c.p;
  if (si == 0) { st.y = c.buf(0, p.i_y0), st.bn = c.bn(0); return st; }
  const int k = (si - 1) / 2;
  st.bn = c.bn(si);
  if (si & 1) { st.y = c.buf(0, p.i_ydw[k]); return st; }
  const Blk& b = c.g.b[k];
  st.y = c.buf(0, p.i_ypw[k]);
  if (b.head) {
    st.has_skip = st.raw = true;
    st.skip = k == 0 ? c.buf(0, p.i_y0) : c.buf(0, p.i_ypw[k - 1]);
    st.skip_bn = c.bn(si - 2);
  } else if (b.skip) {
    st.has_skip = true;
    st.skip = c.buf(0, p.i_ain[k]);
  }
  return st;
}
Stage blur_stage(const Ctx& c, int k) {  // the blurred tensor of a BlurPool block: identity constant block, no residual
  Stage st;
  st.y = c.buf(0, c.p.i_t[k]), st.bn = c.fbuf(0, c.p.i_idbn[k]);
  return st;
}

#define TTK_F(ptr) reinterpret_cast<float*>(ptr)
#define TTK_CF(ptr) reinterpret_cast<const float*>(ptr)

// ---- forward, fp32 ----
int forward_fp32(const Ctx& c) {
  const auto& p = c.p;
  const auto& g = c.g;
  Seq& s = c.s;
  const Args& a = c.a;
  ttk_stream_t st = a.stream;
  const bool training = p.mode == TTK_MOBILENET_TRAIN;
  const int B = p.B;
  float* part = c.fbuf(0, p.i_part);
  auto pivot = [&](int bi) -> const float* { return c.Bf(3 * bi); };
  auto finalize = [&](float* bn, int rows, int C, int64_t count, int gi, int bi) -> int {
    if (training) {
      TTK_SEQ_CALL(s, ttk_bn_fwd_finalize, part, pivot(bi), rows, C, count, c.P(gi), c.P(gi + 1), c.Bf(3 * bi), c.Bf(3 * bi + 1),
                   a.buffers ? static_cast<int64_t*>(a.buffers[3 * bi + 2]) : nullptr, a.momentum, a.eps, bn, st);
    } else {
      TTK_SEQ_CALL(s, ttk_bn_eval_prepare, c.P(gi), c.P(gi + 1), c.Bf(3 * bi), c.Bf(3 * bi + 1), a.eps, C, bn, st);
      TTK_SEQ_CALL(s, ttk_bn_frozen_bound, part, pivot(bi), rows, C, count, bn, st);
    }
    return 0;
  };
  // forward and data-gradient weight operands of the tuned pointwise layers, one call
  {
    const float* w[kMaxBlocks];
    void* prep[kMaxBlocks];
    int ci[kMaxBlocks], co[kMaxBlocks], n = 0;
    for (int k = 0; k < g.n; ++k)
      if (g.b[k].t_pw) {
        w[n] = c.P(3 + 6 * k + 3), ci[n] = g.b[k].cin, co[n] = g.b[k].cout;
        prep[n] = c.buf(0, p.i_prep) ? c.buf(0, p.i_prep) + p.prep_off[k] : nullptr;
        ++n;
      }
    if (n) TTK_SEQ_CALL(s, ttk_pwconv_prepare_weights, n, w, ci, co, prep, st);
  }
  // stem
  const int64_t pix0 = (int64_t)B * g.Ho * g.Wo;
  if (p.c0 == 32) {
    TTK_SEQ_CALL(s, ttk_stem_fwd, a.x, c.P(0), c.buf(0, p.i_y0), part, pivot(0), B, p.H, p.W, 0, st);
    TTK_SEQ_TRY(finalize(c.bn(0), ttk_partial_rows_elementwise(pix0 * 8), 32, pix0, 1, 0));
  } else {
    TTK_SEQ_CALL(s, ttk_anyc_stem_fwd, a.x, c.P(0), TTK_F(c.buf(0, p.i_y0)), part, pivot(0), B, p.H, p.W, p.c0, st);
    TTK_SEQ_TRY(finalize(c.bn(0), ttk_anyc_partial_rows(pix0), p.c0, pix0, 1, 0));
  }
  // one depthwise launch on the output of `sp` -> the rows of partial sums it wrote
  auto dw_fwd = [&](const Stage& sp, char* a_out, const float* w, char* y, const float* pv, int hh, int ww, int C, int stride, int& rows) -> int {
    if (tuned_c(C)) {
      if (sp.raw)
        TTK_SEQ_CALL(s, ttk_dwconv3x3_fwd_rawskip, TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), sp.skip_bn, TTK_F(a_out), w, TTK_F(y), part, pv, B, hh, ww, C, stride, st);
      else
        TTK_SEQ_CALL(s, ttk_dwconv3x3_fwd, TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), TTK_F(a_out), w, TTK_F(y), part, pv, B, hh, ww, C, stride, 0, st);
      rows = ttk_partial_rows_dwconv(B, hh, ww, C, stride, 0);
    } else {
      TTK_SEQ_CALL(s, ttk_anyc_dw_fwd, TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), TTK_F(a_out), w, TTK_F(y), part, pv, B, hh, ww, C, stride, st);
      rows = ttk_anyc_partial_rows((int64_t)B * ((hh - 1) / stride + 1) * ((ww - 1) / stride + 1));
    }
    return 0;
  };
  for (int k = 0; k < g.n; ++k) {
    const Blk& b = g.b[k];
    const int pi = 3 + 6 * k, bi = 1 + 2 * k;
    const Stage prev = stage_of(c, 2 * k);
    char* a_in = b.store_in ? c.buf(0, p.i_ain[k]) : nullptr;
    char* ydw = c.buf(0, p.i_ydw[k]);
    int dw_rows = 0;
    if (b.blur) {
      int unused = 0;
      TTK_SEQ_TRY(dw_fwd(prev, nullptr, c.blurw(k), c.buf(0, p.i_t[k]), nullptr, b.h, b.w, b.cin, b.stride, unused));
      TTK_SEQ_TRY(dw_fwd(blur_stage(c, k), nullptr, c.P(pi), ydw, pivot(bi), b.ho, b.wo, b.cin, 1, dw_rows));
    } else {
      TTK_SEQ_TRY(dw_fwd(prev, a_in, c.P(pi), ydw, pivot(bi), b.h, b.w, b.cin, b.stride, dw_rows));
    }
    float* bn_dw = c.bn(bi);
    TTK_SEQ_TRY(finalize(bn_dw, dw_rows, b.cin, b.M, pi + 1, bi));
    char* ypw = c.buf(0, p.i_ypw[k]);
    int pw_rows;
    if (b.t_pw) {
      TTK_SEQ_CALL(s, ttk_pwconv1x1_fwd, TTK_CF(ydw), bn_dw, nullptr, TTK_F(ypw), part, pivot(bi + 1), b.M, b.cin, b.cout, c.buf(0, p.i_prep) + p.prep_off[k], 0, st);
      pw_rows = ttk_partial_rows_pwconv(b.M, b.cin, b.cout, 0);
    } else {
      TTK_SEQ_CALL(s, ttk_anyc_pw_fwd, TTK_CF(ydw), bn_dw, c.P(pi + 3), TTK_F(ypw), part, pivot(bi + 1), b.M, b.cin, b.cout, st);
      pw_rows = ttk_partial_rows_gemm(b.M);
    }
    TTK_SEQ_TRY(finalize(c.bn(bi + 1), pw_rows, b.cout, b.M, pi + 4, bi + 1));
  }
  const Stage last = stage_of(c, 2 * g.n);
  const int C = g.b[g.n - 1].cout, HW = g.hl * g.wl;
  if (tuned_c(C) && last.raw)
    TTK_SEQ_CALL(s, ttk_avgpool_fwd_rawskip, TTK_CF(last.y), last.bn, TTK_CF(last.skip), last.skip_bn, a.feat, B, HW, C, st);
  else if (tuned_c(C))
    TTK_SEQ_CALL(s, ttk_avgpool_fwd, TTK_CF(last.y), last.bn, TTK_CF(last.skip), a.feat, B, HW, C, 0, st);
  else
    TTK_SEQ_CALL(s, ttk_anyc_avgpool_fwd, TTK_CF(last.y), last.bn, TTK_CF(last.skip), a.feat, B, HW, C, st);
  return 0;
}

// ---- forward, bf16-compute ----
int forward_bc(const Ctx& c) {
  const auto& p = c.p;
  const auto& g = c.g;
  Seq& s = c.s;
  const Args& a = c.a;
  ttk_stream_t st = a.stream;
  const bool training = p.mode == TTK_MOBILENET_TRAIN;
  const int B = p.B, kBf = TTK_STORE_ACT_BF16 | TTK_STORE_GRAD_BF16;
  float* part = c.fbuf(0, p.i_part);
  auto pivot = [&](int bi) -> const float* { return c.Bf(3 * bi); };
  auto finalize = [&](float* bn, int rows, int C, int64_t count, int gi, int bi) -> int {
    if (training)
      TTK_SEQ_CALL(s, ttk_bn_fwd_finalize, part, pivot(bi), rows, C, count, c.P(gi), c.P(gi + 1), c.Bf(3 * bi), c.Bf(3 * bi + 1),
                   a.buffers ? static_cast<int64_t*>(a.buffers[3 * bi + 2]) : nullptr, a.momentum, a.eps, bn, st);
    else
      TTK_SEQ_CALL(s, ttk_bn_eval_prepare, c.P(gi), c.P(gi + 1), c.Bf(3 * bi), c.Bf(3 * bi + 1), a.eps, C, bn, st);
    return 0;
  };
  {
    const float* w[kMaxBlocks];
    void* prep[kMaxBlocks];
    int ci[kMaxBlocks], co[kMaxBlocks];
    for (int k = 0; k < g.n; ++k) {
      w[k] = c.P(3 + 6 * k + 3), ci[k] = g.b[k].cin, co[k] = g.b[k].cout;
      prep[k] = c.buf(0, p.i_prep) ? c.buf(0, p.i_prep) + p.prep_off[k] : nullptr;
    }
    TTK_SEQ_CALL(s, ttk_bc_prepare_weights, g.n, w, ci, co, prep, st);
  }
  const int64_t pix0 = (int64_t)B * g.Ho * g.Wo;
  TTK_SEQ_CALL(s, ttk_stem_fwd, a.x, c.P(0), c.buf(0, p.i_y0), part, pivot(0), B, p.H, p.W, kBf, st);
  TTK_SEQ_TRY(finalize(c.bn(0), ttk_partial_rows_elementwise(pix0 * 8), 32, pix0, 1, 0));
  for (int k = 0; k < g.n; ++k) {
    const Blk& b = g.b[k];
    const int pi = 3 + 6 * k, bi = 1 + 2 * k;
    const Stage prev = stage_of(c, 2 * k);
    char* a_in = b.store_in ? c.buf(0, p.i_ain[k]) : nullptr;
    char* ydw = c.buf(0, p.i_ydw[k]);
    int dw_rows;
    if (b.blur) {
      char* t = c.buf(0, p.i_t[k]);
      TTK_SEQ_CALL(s, ttk_bc_dw_fwd, prev.y, prev.bn, prev.skip, nullptr, c.blurw(k), t, part, nullptr, B, b.h, b.w, b.cin, b.stride, st);
      TTK_SEQ_CALL(s, ttk_bc_dw_fwd, t, c.fbuf(0, p.i_idbn[k]), nullptr, nullptr, c.P(pi), ydw, part, pivot(bi), B, b.ho, b.wo, b.cin, 1, st);
      dw_rows = ttk_bc_partial_rows_dw(B, b.ho, b.wo, b.cin, 1, 0);
    } else {
      TTK_SEQ_CALL(s, ttk_bc_dw_fwd, prev.y, prev.bn, prev.skip, a_in, c.P(pi), ydw, part, pivot(bi), B, b.h, b.w, b.cin, b.stride, st);
      dw_rows = ttk_bc_partial_rows_dw(B, b.h, b.w, b.cin, b.stride, 0);
    }
    float* bn_dw = c.bn(bi);
    TTK_SEQ_TRY(finalize(bn_dw, dw_rows, b.cin, b.M, pi + 1, bi));
    char* ypw = c.buf(0, p.i_ypw[k]);
    TTK_SEQ_CALL(s, ttk_bc_pw_fwd, ydw, bn_dw, c.buf(0, p.i_prep) + p.prep_off[k], ypw, part, pivot(bi + 1), b.M, b.cin, b.cout, st);
    TTK_SEQ_TRY(finalize(c.bn(bi + 1), ttk_bc_partial_rows_pw(b.M, b.cin, b.cout), b.cout, b.M, pi + 4, bi + 1));
  }
  const Stage last = stage_of(c, 2 * g.n);
  TTK_SEQ_CALL(s, ttk_bc_avgpool_fwd, last.y, last.bn, last.skip, a.feat, B, g.hl * g.wl, g.b[g.n - 1].cout, st);
  return 0;
}

// the weight-gradient scratch of the fp32 backward: bytes of the four buffers, by the rules of mobilenet_v1._backward_impl
struct ScratchFp32 { uint64_t wg = 0, pw = 0, dwrows = 0, any = 0, pw_need = 0; };
ScratchFp32 scratch_fp32(const ttk_mobilenet_plan& p, const Geo& g) {
  ScratchFp32 r;
  const int B = p.B;
  const bool frozen = p.mode == TTK_MOBILENET_FROZEN;
  auto up = [](uint64_t& m, uint64_t v) { if (v > m) m = v; };
  if (p.deterministic) {
    up(r.wg, ttk_stem_wgrad_partial_bytes());
    for (int k = 0; k < g.n; ++k) {
      const Blk& b = g.b[k];
      if (b.t_pw) up(r.wg, ttk_pwconv_wgrad_partial_bytes(b.M, b.cin, b.cout)), up(r.wg, ttk_pwconv1x1_bwd_fused_partial_bytes(b.M, b.cin, b.cout));
      if (b.t_in) {
        up(r.wg, (uint64_t)ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 1) * 9 * b.cin * 4);
        if (b.blur) up(r.wg, (uint64_t)ttk_partial_rows_dwconv(B, b.ho, b.wo, b.cin, 1, 1) * 9 * b.cin * 4);
      }
    }
    r.wg = r.wg / 4 * 4;
  }
  for (int k = 0; k < g.n; ++k)
    if (g.b[k].t_pw) up(r.pw_need, ttk_pwconv_wgrad_scratch_bytes(g.b[k].M, g.b[k].cin, g.b[k].cout));
  if (!(p.deterministic && r.wg >= r.pw_need)) r.pw = r.pw_need / 4 * 4;
  if (!p.deterministic && !frozen)
    for (int k = 0; k < g.n; ++k)
      if (!g.b[k].blur && g.b[k].t_in) up(r.dwrows, (uint64_t)ttk_partial_rows_dwconv(B, g.b[k].h, g.b[k].w, g.b[k].cin, g.b[k].stride, 1) * 9 * g.b[k].cin * 4);
  if (p.c0 != 32) up(r.any, ttk_anyc_stem_wgrad_scratch_bytes(B, p.H, p.W, p.c0));
  for (int k = 0; k < g.n; ++k) {
    const Blk& b = g.b[k];
    if (!b.t_in) up(r.any, b.blur ? ttk_anyc_dw_wgrad_scratch_bytes(B, b.ho, b.wo, b.cin) : ttk_anyc_dw_wgrad_scratch_bytes(B, b.h, b.w, b.cin));
    if (!b.t_pw) up(r.any, ttk_anyc_pw_wgrad_scratch_bytes(b.M, b.cin, b.cout));
  }
  r.any = r.any / 4 * 4;
  return r;
}

void announce(const Ctx& c, int first, int last) {
  if (!c.s.dry && c.a.on_ready) c.a.on_ready(c.a.user, first, last);
}

// ---- backward, fp32 ----
int backward_fp32(const Ctx& c) {
  const auto& p = c.p;
  const auto& g = c.g;
  Seq& s = c.s;
  const Args& a = c.a;
  ttk_stream_t st = a.stream;
  const int B = p.B, nparams = p.nparams;
  const bool frozen = p.mode == TTK_MOBILENET_FROZEN, det = p.deterministic != 0;
  float* part = c.fbuf(0, p.i_part);
  float* wg = c.fbuf(1, p.i_wg);  // deterministic mode: every weight-gradient reduction stores rows here, folded in a fixed order
  const bool has_wg = det;
  float* pw_scratch = (has_wg && p.i_pw < 0) ? wg : c.fbuf(1, p.i_pw);
  float* dw_rows = has_wg ? wg : c.fbuf(1, p.i_dwrows);
  float* any_scratch = c.fbuf(1, p.i_any);
  auto bwd_finalize = [&](float* bn, int C, int rows, int64_t count, int gi) -> int {
    if (frozen)
      TTK_SEQ_CALL(s, ttk_bn_bwd_frozen, bn, C, st);
    else
      TTK_SEQ_CALL(s, ttk_bn_bwd_finalize, part, rows, C, count, c.P(gi), bn, c.grad(gi), c.grad(gi + 1), 0, st);
    return 0;
  };
  const Stage last = stage_of(c, 2 * g.n);
  const int C = g.b[g.n - 1].cout, HW = g.hl * g.wl;
  char* gcur = c.buf(1, p.i_g[(g.n - 1) & 1]);
  if (tuned_c(C)) {
    if (last.raw)
      TTK_SEQ_CALL(s, ttk_avgpool_bwd_rawskip, a.gfeat, TTK_CF(last.y), last.bn, TTK_CF(last.skip), last.skip_bn, TTK_F(gcur), part, B, HW, C, st);
    else
      TTK_SEQ_CALL(s, ttk_avgpool_bwd, a.gfeat, TTK_CF(last.y), last.bn, TTK_CF(last.skip), TTK_F(gcur), part, B, HW, C, 0, st);
    TTK_SEQ_TRY(bwd_finalize(last.bn, C, ttk_partial_rows_elementwise((int64_t)B * HW * (C / 4)), (int64_t)B * HW, nparams - 2));
  } else {
    TTK_SEQ_CALL(s, ttk_anyc_avgpool_bwd, a.gfeat, TTK_CF(last.y), last.bn, TTK_CF(last.skip), TTK_F(gcur), part, B, HW, C, st);
    TTK_SEQ_TRY(bwd_finalize(last.bn, C, ttk_anyc_partial_rows((int64_t)B * HW), (int64_t)B * HW, nparams - 2));
  }
  // one tuned depthwise data-gradient launch into the output of stage `sp` (its residual operand stored or raw)
  auto dw_bwd = [&](const char* g_dw, const Stage& sd, const float* w, const char* skip_grad, const Stage& sp, bool stored, const char* a_in, char* g_prev,
                    float* dw, int acc, float* rows, int hh, int ww, int Cc, int stride) -> int {
    if (sp.raw && !stored)
      TTK_SEQ_CALL(s, ttk_dwconv3x3_bwd_data_rawskip, TTK_CF(g_dw), TTK_CF(sd.y), sd.bn, w, TTK_CF(skip_grad), TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), sp.skip_bn, TTK_F(g_prev),
                   part, dw, acc, rows, B, hh, ww, Cc, stride, st);
    else  // (a stored a_in stands for the whole block input: the residual operand, stored or raw, is not read)
      TTK_SEQ_CALL(s, ttk_dwconv3x3_bwd_data, TTK_CF(g_dw), TTK_CF(sd.y), sd.bn, w, TTK_CF(skip_grad), TTK_CF(sp.y), sp.bn, sp.raw ? nullptr : TTK_CF(sp.skip), TTK_CF(a_in),
                   TTK_F(g_prev), part, dw, acc, rows, B, hh, ww, Cc, stride, 0, st);
    return 0;
  };
  for (int k = g.n - 1; k >= 0; --k) {
    const Blk& b = g.b[k];
    const int pi = 3 + 6 * k;
    const Stage sp = stage_of(c, 2 * k), sd = stage_of(c, 2 * k + 1), sw = stage_of(c, 2 * k + 2);
    // (dry runs have no pointers: whether the block input was stored is the plan's flag)
    const bool stored = b.store_in;
    const char* a_in = stored ? c.buf(0, p.i_ain[k]) : nullptr;
    const float* w_dw = c.P(pi);
    const float* w_pw = c.P(pi + 3);
    float* dW = c.grad(pi + 3);
    char* g_dw = c.buf(1, p.i_gdw);
    char* prepk = c.buf(0, p.i_prep) ? c.buf(0, p.i_prep) + p.prep_off[k] : nullptr;
    const int fused_rows = b.t_pw ? ttk_pwconv1x1_bwd_fused_rows(b.M, b.cin, b.cout) : 0;
    // -- pointwise: weight gradient, data gradient (+ bn_dw backward sums)
    if (!b.t_pw) {
      TTK_SEQ_CALL(s, ttk_anyc_pw_bwd_weight, TTK_CF(gcur), TTK_CF(sw.y), sw.bn, TTK_CF(sd.y), sd.bn, dW, 0, any_scratch, b.M, b.cin, b.cout, st);
      TTK_SEQ_CALL(s, ttk_anyc_pw_bwd_data, TTK_CF(gcur), TTK_CF(sw.y), sw.bn, w_pw, TTK_CF(sd.y), sd.bn, TTK_F(g_dw), part, b.M, b.cin, b.cout, st);
      TTK_SEQ_TRY(bwd_finalize(sd.bn, b.cin, ttk_partial_rows_gemm(b.M), b.M, pi + 1));
    } else if (fused_rows > 0) {
      TTK_SEQ_CALL(s, ttk_pwconv1x1_bwd_fused, TTK_CF(gcur), TTK_CF(sw.y), sw.bn, w_pw, prepk, TTK_CF(sd.y), sd.bn, TTK_F(g_dw), dW, wg, part, b.M, b.cin, b.cout, st);
      TTK_SEQ_TRY(bwd_finalize(sd.bn, b.cin, fused_rows, b.M, pi + 1));
    } else {
      float* partial = has_wg ? wg : (ttk_pwconv_wgrad_scratch_bytes(b.M, b.cin, b.cout) ? pw_scratch : nullptr);
      TTK_SEQ_CALL(s, ttk_pwconv1x1_bwd_weight, TTK_CF(gcur), TTK_CF(sw.y), sw.bn, TTK_CF(sd.y), sd.bn, dW, partial, b.M, b.cin, b.cout, 0, st);
      TTK_SEQ_CALL(s, ttk_pwconv1x1_bwd_data, TTK_CF(gcur), TTK_CF(sw.y), sw.bn, nullptr, TTK_CF(sd.y), sd.bn, TTK_F(g_dw), part, b.M, b.cin, b.cout, prepk, 0, st);
      TTK_SEQ_TRY(bwd_finalize(sd.bn, b.cin, ttk_partial_rows_pwconv(b.M, b.cout, b.cin, 1), b.M, pi + 1));
    }
    // -- depthwise: data gradient (+ residual gradient, + producer's bn sums) with the fused weight gradient
    float* dWd = c.grad(pi);
    char* g_prev = c.buf(1, p.i_g[(k + 1) & 1]);
    const int gi_prev = k > 0 ? pi - 2 : 1;
    const int64_t pix_in = (int64_t)B * b.h * b.w;
    const char* skip_grad = b.skip ? gcur : nullptr;
    if (!b.t_in) {
      if (b.blur) {
        const Stage stt = blur_stage(c, k);
        char* g_t = c.buf(1, p.i_gt);
        TTK_SEQ_CALL(s, ttk_anyc_dw_bwd_data, TTK_CF(g_dw), TTK_CF(sd.y), sd.bn, w_dw, nullptr, TTK_CF(stt.y), stt.bn, nullptr, nullptr, TTK_F(g_t), part, dWd, 0,
                     any_scratch, B, b.ho, b.wo, b.cin, 1, st);
        TTK_SEQ_CALL(s, ttk_bn_bwd_frozen, stt.bn, b.cin, st);
        TTK_SEQ_CALL(s, ttk_anyc_dw_bwd_data, TTK_CF(g_t), TTK_CF(stt.y), stt.bn, c.blurw(k), nullptr, TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), nullptr, TTK_F(g_prev), part,
                     nullptr, 0, nullptr, B, b.h, b.w, b.cin, b.stride, st);
      } else {
        TTK_SEQ_CALL(s, ttk_anyc_dw_bwd_data, TTK_CF(g_dw), TTK_CF(sd.y), sd.bn, w_dw, TTK_CF(skip_grad), TTK_CF(sp.y), sp.bn, TTK_CF(sp.skip), TTK_CF(a_in), TTK_F(g_prev), part,
                     dWd, 0, any_scratch, B, b.h, b.w, b.cin, b.stride, st);
      }
      TTK_SEQ_TRY(bwd_finalize(sp.bn, b.cin, ttk_anyc_partial_rows(pix_in), pix_in, gi_prev));
    } else if (b.blur) {
      const Stage stt = blur_stage(c, k);
      char* g_t = c.buf(1, p.i_gt);
      TTK_SEQ_TRY(dw_bwd(g_dw, sd, w_dw, nullptr, stt, false, nullptr, g_t, dWd, 1, wg, b.ho, b.wo, b.cin, 1));
      TTK_SEQ_CALL(s, ttk_bn_bwd_frozen, stt.bn, b.cin, st);
      TTK_SEQ_TRY(dw_bwd(g_t, stt, c.blurw(k), nullptr, sp, false, nullptr, g_prev, nullptr, 0, nullptr, b.h, b.w, b.cin, b.stride));
      TTK_SEQ_TRY(bwd_finalize(sp.bn, b.cin, ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 1), pix_in, gi_prev));
    } else if (!det && !frozen) {
      // workgroup rows, folded by the launch that finalises the producer's BatchNorm backward
      const int rows = ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 1);
      TTK_SEQ_TRY(dw_bwd(g_dw, sd, w_dw, skip_grad, sp, stored, a_in, g_prev, dWd, 2, dw_rows, b.h, b.w, b.cin, b.stride));
      TTK_SEQ_CALL(s, ttk_bc_bn_bwd_finalize_fold, part, rows, b.cin, pix_in, c.P(gi_prev), sp.bn, c.grad(gi_prev), c.grad(gi_prev + 1), 0, dw_rows, rows,
                   (int64_t)9 * b.cin, dWd, 1, st);
    } else {
      TTK_SEQ_TRY(dw_bwd(g_dw, sd, w_dw, skip_grad, sp, stored, a_in, g_prev, dWd, 1, wg, b.h, b.w, b.cin, b.stride));
      TTK_SEQ_TRY(bwd_finalize(sp.bn, b.cin, ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 1), pix_in, gi_prev));
    }
    gcur = g_prev;
    announce(c, pi, pi + 6);  // this block's conv + bn_dw gradients and its own bn_sep gradients are final
  }
  const Stage s0 = stage_of(c, 0);
  if (p.c0 == 32)
    TTK_SEQ_CALL(s, ttk_stem_bwd_weight, gcur, s0.y, s0.bn, a.x, c.grad(0), 1, wg, B, p.H, p.W, 0, st);
  else
    TTK_SEQ_CALL(s, ttk_anyc_stem_bwd_weight, TTK_CF(gcur), TTK_CF(s0.y), s0.bn, a.x, c.grad(0), 0, any_scratch, B, p.H, p.W, p.c0, st);
  announce(c, 0, 3);
  return 0;
}

uint64_t scratch_bc(const ttk_mobilenet_plan& p, const Geo& g) {
  uint64_t need = 0;
  auto up = [&](uint64_t v) { if (v > need) need = v; };
  for (int k = 0; k < g.n; ++k) {
    const Blk& b = g.b[k];
    up(ttk_bc_pw_wgrad_scratch_bytes(b.M, b.cin, b.cout)), up(ttk_bc_pw_bwd_fused_scratch_bytes(b.M, b.cin, b.cout));
    up((uint64_t)ttk_bc_partial_rows_dw(p.B, b.h, b.w, b.cin, b.stride, 1) * 9 * b.cin * 4);
    if (b.blur) up((uint64_t)ttk_bc_partial_rows_dw(p.B, b.ho, b.wo, b.cin, 1, 1) * 9 * b.cin * 4);
  }
  if (p.deterministic) up(ttk_stem_wgrad_partial_bytes());
  return need / 4 * 4;
}

// ---- backward, bf16-compute ----
int backward_bc(const Ctx& c) {
  const auto& p = c.p;
  const auto& g = c.g;
  Seq& s = c.s;
  const Args& a = c.a;
  ttk_stream_t st = a.stream;
  const int B = p.B, nparams = p.nparams, kBf = TTK_STORE_ACT_BF16 | TTK_STORE_GRAD_BF16;
  const bool frozen = p.mode == TTK_MOBILENET_FROZEN, det = p.deterministic != 0;
  float* part = c.fbuf(0, p.i_part);
  float* scratch = c.fbuf(1, p.i_wg);
  auto bwd_finalize = [&](float* bn, int C, int rows, int64_t count, int gi) -> int {
    if (frozen)
      TTK_SEQ_CALL(s, ttk_bn_bwd_frozen, bn, C, st);
    else
      TTK_SEQ_CALL(s, ttk_bn_bwd_finalize, part, rows, C, count, c.P(gi), bn, c.grad(gi), c.grad(gi + 1), 0, st);
    return 0;
  };
  const Stage last = stage_of(c, 2 * g.n);
  const int C = g.b[g.n - 1].cout, HW = g.hl * g.wl;
  char* gcur = c.buf(1, p.i_g[(g.n - 1) & 1]);
  TTK_SEQ_CALL(s, ttk_bc_avgpool_bwd, a.gfeat, last.y, last.bn, last.skip, gcur, part, B, HW, C, st);
  TTK_SEQ_TRY(bwd_finalize(last.bn, C, ttk_bc_partial_rows_pool(B, HW, C), (int64_t)B * HW, nparams - 2));
  for (int k = g.n - 1; k >= 0; --k) {
    const Blk& b = g.b[k];
    const int pi = 3 + 6 * k;
    const Stage sp = stage_of(c, 2 * k), sd = stage_of(c, 2 * k + 1), sw = stage_of(c, 2 * k + 2);
    const char* a_in = b.store_in ? c.buf(0, p.i_ain[k]) : nullptr;
    const float* w_dw = c.P(pi);
    char* g_dw = c.buf(1, p.i_gdw);
    char* prepk = c.buf(0, p.i_prep) ? c.buf(0, p.i_prep) + p.prep_off[k] : nullptr;
    const int fused_rows = ttk_bc_pw_bwd_fused_rows(b.M, b.cin, b.cout);
    const bool defer = !frozen && fused_rows > 0;  // the slice tiles are folded by the launch that finalises bn_dw's backward
    float* dWp = defer ? nullptr : c.grad(pi + 3);
    int rows, slices;
    if (fused_rows > 0) {
      TTK_SEQ_CALL(s, ttk_bc_pw_bwd_fused, gcur, sw.y, sw.bn, prepk, sd.y, sd.bn, g_dw, dWp, scratch, part, b.M, b.cin, b.cout, st);
      rows = slices = fused_rows;
    } else {
      TTK_SEQ_CALL(s, ttk_bc_pw_bwd_weight, gcur, sw.y, sw.bn, sd.y, sd.bn, dWp, scratch, b.M, b.cin, b.cout, st);
      TTK_SEQ_CALL(s, ttk_bc_pw_bwd_data, gcur, sw.y, sw.bn, prepk, sd.y, sd.bn, g_dw, part, b.M, b.cin, b.cout, st);
      rows = ttk_bc_partial_rows_pw(b.M, b.cout, b.cin), slices = ttk_bc_pw_wgrad_slices(b.M, b.cin, b.cout);
    }
    if (defer)
      TTK_SEQ_CALL(s, ttk_bc_bn_bwd_finalize_fold, part, rows, b.cin, b.M, c.P(pi + 1), sd.bn, c.grad(pi + 1), c.grad(pi + 2), 0, scratch, slices,
                   (int64_t)b.cin * b.cout, c.grad(pi + 3), 1, st);
    else
      TTK_SEQ_TRY(bwd_finalize(sd.bn, b.cin, rows, b.M, pi + 1));
    float* dWd = c.grad(pi);
    char* g_prev = c.buf(1, p.i_g[(k + 1) & 1]);
    const int gi = k > 0 ? pi - 2 : 1;
    const int64_t pix_in = (int64_t)B * b.h * b.w;
    const char* skip_grad = b.skip ? gcur : nullptr;
    const int drows = ttk_bc_partial_rows_dw(B, b.h, b.w, b.cin, b.stride, 1);
    if (b.blur) {
      const Stage stt = blur_stage(c, k);
      char* g_t = c.buf(1, p.i_gt);
      TTK_SEQ_CALL(s, ttk_bc_dw_bwd_data, g_dw, sd.y, sd.bn, w_dw, nullptr, stt.y, stt.bn, nullptr, nullptr, g_t, part, dWd, 1, scratch, B, b.ho, b.wo,
                   b.cin, 1, st);
      TTK_SEQ_CALL(s, ttk_bn_bwd_frozen, stt.bn, b.cin, st);
      TTK_SEQ_CALL(s, ttk_bc_dw_bwd_data, g_t, stt.y, stt.bn, c.blurw(k), nullptr, sp.y, sp.bn, sp.skip, nullptr, g_prev, part, nullptr, 0, nullptr, B,
                   b.h, b.w, b.cin, b.stride, st);
      TTK_SEQ_TRY(bwd_finalize(sp.bn, b.cin, drows, pix_in, gi));
    } else if (frozen) {
      TTK_SEQ_CALL(s, ttk_bc_dw_bwd_data, g_dw, sd.y, sd.bn, w_dw, skip_grad, sp.y, sp.bn, sp.skip, a_in, g_prev, part, dWd, 1, scratch, B, b.h, b.w,
                   b.cin, b.stride, st);
      TTK_SEQ_TRY(bwd_finalize(sp.bn, b.cin, drows, pix_in, gi));
    } else {
      TTK_SEQ_CALL(s, ttk_bc_dw_bwd_data, g_dw, sd.y, sd.bn, w_dw, skip_grad, sp.y, sp.bn, sp.skip, a_in, g_prev, part, dWd, 2, scratch, B, b.h, b.w,
                   b.cin, b.stride, st);
      TTK_SEQ_CALL(s, ttk_bc_bn_bwd_finalize_fold, part, drows, b.cin, pix_in, c.P(gi), sp.bn, c.grad(gi), c.grad(gi + 1), 0, scratch, drows,
                   (int64_t)9 * b.cin, dWd, 1, st);
    }
    gcur = g_prev;
    announce(c, pi, pi + 6);
  }
  const Stage s0 = stage_of(c, 0);
  TTK_SEQ_CALL(s, ttk_stem_bwd_weight, gcur, s0.y, s0.bn, a.x, c.grad(0), 1, det ? scratch : nullptr, B, p.H, p.W, kBf, st);
  announce(c, 0, 3);
  return 0;
}

int emit(const ttk_mobilenet_plan& p, const Args& a, Seq& s, int backward) {
  Geo g;
  geometry(p, g);
  const Offsets o(p);
  const Ctx c{p, g, a, s, o};
  if (backward) return g.bc ? backward_bc(c) : backward_fp32(c);
  return g.bc ? forward_bc(c) : forward_fp32(c);
}

// rows of the [rows][2][C] scratch of partial sums every layer shares: the largest need, in floats
// (mobilenet_v1._part_buffer / _mobilenet_bc.part_buffer); false: a row count came back negative (a shape its kernel does not take)
bool part_floats(const ttk_mobilenet_plan& p, const Geo& g, uint64_t& need) {
  bool ok = true;
  need = 0;
  auto up = [&](int64_t rows, int C) {
    if (rows < 0) ok = false;
    else if ((uint64_t)rows * 2 * C > need) need = (uint64_t)rows * 2 * C;
  };
  const int B = p.B;
  const int64_t pix0 = (int64_t)B * g.Ho * g.Wo;
  if (g.bc) {
    up(ttk_partial_rows_elementwise(pix0 * 8), 32);
    for (int k = 0; k < g.n; ++k) {
      const Blk& b = g.b[k];
      up(ttk_bc_partial_rows_dw(B, b.h, b.w, b.cin, b.stride, 1), b.cin), up(ttk_bc_partial_rows_dw(B, b.h, b.w, b.cin, b.stride, 0), b.cin);
      if (b.blur && b.stride == 2) up(ttk_bc_partial_rows_dw(B, b.ho, b.wo, b.cin, 1, 0), b.cin), up(ttk_bc_partial_rows_dw(B, b.ho, b.wo, b.cin, 1, 1), b.cin);
      up(ttk_bc_partial_rows_pw(b.M, b.cin, b.cout), b.cout), up(ttk_bc_partial_rows_pw(b.M, b.cout, b.cin), b.cin);
      up(ttk_bc_pw_bwd_fused_rows(b.M, b.cin, b.cout), b.cin);
      up(ttk_bc_partial_rows_pool(B, b.ho * b.wo, b.cout), b.cout);
    }
    return ok;
  }
  up(p.c0 == 32 ? ttk_partial_rows_elementwise(pix0 * 8) : ttk_anyc_partial_rows(pix0), p.c0);
  for (int k = 0; k < g.n; ++k) {
    const Blk& b = g.b[k];
    if (b.t_in) {
      up(ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 1), b.cin), up(ttk_partial_rows_dwconv(B, b.h, b.w, b.cin, b.stride, 0), b.cin);
      if (b.blur && b.stride == 2) up(ttk_partial_rows_dwconv(B, b.ho, b.wo, b.cin, 1, 0), b.cin), up(ttk_partial_rows_dwconv(B, b.ho, b.wo, b.cin, 1, 1), b.cin);
    } else {
      up(ttk_anyc_partial_rows((int64_t)B * b.h * b.w), b.cin);
    }
    if (b.t_pw)
      up(ttk_partial_rows_pwconv(b.M, b.cin, b.cout, 0), b.cout), up(ttk_partial_rows_pwconv(b.M, b.cout, b.cin, 1), b.cin);
    else
      up(ttk_partial_rows_gemm(b.M), b.cin > b.cout ? b.cin : b.cout);
    if (b.t_out)
      up(ttk_partial_rows_elementwise(b.M * (b.cout / 4)), b.cout);
    else
      up(ttk_anyc_partial_rows(b.M), b.cout);
  }
  return ok;
}

struct Table {
  ttk_mobilenet_plan& p;
  int which;
  uint64_t cur = 0;
  bool overflow = false;
  int add(uint64_t bytes) {
    if (!bytes) return -1;
    if (p.nbuf[which] >= TTK_MOBILENET_MAX_BUFFERS) { overflow = true; return -1; }
    const int i = p.nbuf[which]++;
    p.buf_off[which][i] = cur, p.buf_bytes[which][i] = bytes;
    cur += align256(bytes);
    return i;
  }
};

int plan_fill(ttk_mobilenet_plan& p, const int* cin, const int* cout, const int* stride, const int* blur) {
  const int B = p.B, H = p.H, W = p.W, c0 = p.c0, n = p.nblocks;
  TTK_REQUIRE(n >= 1 && n <= kMaxBlocks, "mobilenet_plan_init: nblocks = %d (1..%d blocks)", n, kMaxBlocks);
  TTK_REQUIRE(cin && cout && stride, "mobilenet_plan_init: cin, cout and stride must not be NULL");
  TTK_REQUIRE(B >= 1 && H >= 1 && W >= 1, "mobilenet_plan_init: B = %d, H = %d, W = %d must be positive", B, H, W);
  TTK_REQUIRE(p.mode == TTK_MOBILENET_TRAIN || p.mode == TTK_MOBILENET_FROZEN || p.mode == TTK_MOBILENET_EVAL, "mobilenet_plan_init: mode = %d (TTK_MOBILENET_TRAIN, _FROZEN or _EVAL)", p.mode);
  TTK_REQUIRE(p.precision == TTK_MOBILENET_FP32 || p.precision == TTK_MOBILENET_BF16_COMPUTE, "mobilenet_plan_init: precision = %d (TTK_MOBILENET_FP32 or _BF16_COMPUTE)", p.precision);
  TTK_REQUIRE(p.deterministic == 0 || p.deterministic == 1, "mobilenet_plan_init: deterministic = %d (0 or 1)", p.deterministic);
  TTK_REQUIRE(anyc_c(c0), "mobilenet_plan_init: c0 = %d (32 for the tuned stem, or a multiple of 8 in 8..2048)", c0);
  for (int k = 0; k < n; ++k) {
    p.cin[k] = cin[k], p.cout[k] = cout[k], p.stride[k] = stride[k], p.blur[k] = blur ? (blur[k] != 0) : 0;
    TTK_REQUIRE(stride[k] == 1 || stride[k] == 2, "mobilenet_plan_init: stride[%d] = %d (1 or 2)", k, stride[k]);
    TTK_REQUIRE(anyc_c(cin[k]) && anyc_c(cout[k]), "mobilenet_plan_init: block %d: cin = %d, cout = %d (powers of two in 32..1024 for the tuned kernels, multiples of 8 in 8..2048 otherwise)", k, cin[k], cout[k]);
    TTK_REQUIRE(cin[k] == (k ? cout[k - 1] : c0), "mobilenet_plan_init: cin[%d] = %d does not continue the %d channels before it", k, cin[k], k ? cout[k - 1] : c0);
    TTK_REQUIRE(!p.blur[k] || stride[k] == 2, "mobilenet_plan_init: blur[%d] is set on a block of stride 1 (BlurPool replaces the stride of a strided block)", k);
  }
  const bool bc = p.precision == TTK_MOBILENET_BF16_COMPUTE;
  if (bc) {
    bool ref = n == 13 && c0 == 32;
    for (int k = 0; ref && k < 13; ++k) ref = cin[k] == kRefCin[k] && cout[k] == kRefCout[k] && stride[k] == kRefStride[k];
    TTK_REQUIRE(ref, "mobilenet_plan_init: precision bf16-compute is built for the width 1.0 block table only (64-channel blocks): use TTK_MOBILENET_FP32 for this cin / cout / stride table");
  }
  Geo g;
  geometry(p, g);
  // 32-bit indexing: pixel counts and the largest activation tensor
  TTK_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "mobilenet_plan_init: B * H * W = %lld pixels exceed 32-bit indexing", (long long)B * H * W);
  int64_t big = (int64_t)B * g.Ho * g.Wo * c0;
  for (int k = 0; k < n; ++k) {
    const Blk& b = g.b[k];
    const int64_t in = (int64_t)B * b.h * b.w * b.cin, mid = b.M * b.cin, out = b.M * b.cout;
    big = in > big ? in : big, big = mid > big ? mid : big, big = out > big ? out : big;
  }
  TTK_REQUIRE(big < ((int64_t)1 << 31), "mobilenet_plan_init: B = %d at %d x %d: the largest activation has %lld elements, beyond 32-bit indexing", B, H, W, (long long)big);

  const int es = kEs[bc ? 1 : 0];
  p.nparams = 3 + 6 * n, p.nbuffers = 3 * (1 + 2 * n);
  uint64_t part = 0;
  TTK_REQUIRE(part_floats(p, g, part), "mobilenet_plan_init: a layer of the cin / cout table has a shape its kernel family does not take");
  // ---- forward workspace
  Table f{p, 0};
  p.i_part = f.add(part * 4);
  uint64_t bn_floats = (uint64_t)TTK_BN_ROWS * c0;
  for (int k = 0; k < n; ++k) bn_floats += (uint64_t)TTK_BN_ROWS * (cin[k] + cout[k]);
  p.i_bn = f.add(bn_floats * 4);
  uint64_t prep = 0;
  for (int k = 0; k < n; ++k) {
    p.prep_off[k] = prep;
    p.prep_bytes[k] = bc ? ttk_bc_prepared_bytes(cin[k], cout[k]) : (g.b[k].t_pw ? ttk_pwconv_prepared_bytes(cin[k], cout[k]) : 0);
    prep += p.prep_bytes[k];
  }
  p.i_prep = f.add(prep);
  p.i_y0 = f.add((uint64_t)B * g.Ho * g.Wo * c0 * es);
  for (int k = 0; k < n; ++k) {
    const Blk& b = g.b[k];
    p.i_ain[k] = b.store_in ? f.add((uint64_t)B * b.h * b.w * b.cin * es) : -1;
    p.i_t[k] = b.blur ? f.add((uint64_t)b.M * b.cin * es) : -1;
    p.i_idbn[k] = b.blur ? f.add((uint64_t)TTK_BN_ROWS * b.cin * 4) : -1;
    p.i_ydw[k] = f.add((uint64_t)b.M * b.cin * es);
    p.i_ypw[k] = f.add((uint64_t)b.M * b.cout * es);
  }
  for (int k = n; k < kMaxBlocks; ++k) p.i_ain[k] = p.i_t[k] = p.i_idbn[k] = p.i_ydw[k] = p.i_ypw[k] = -1;
  p.ws_bytes[0] = f.cur;
  // ---- backward workspace and gradient arena
  Table bw{p, 1};
  p.i_g[0] = p.i_g[1] = p.i_gdw = p.i_gt = p.i_wg = p.i_pw = p.i_dwrows = p.i_any = -1;
  p.arena_floats = 0;
  if (p.mode != TTK_MOBILENET_EVAL) {
    // the gradient of block k's output lives in buffer k & 1, that of its input (block k - 1's output; the stem's for k = 0) in the other one
    uint64_t gb[2] = {0, 0}, gdw = 0, gt = 0;
    auto up = [](uint64_t& m, uint64_t v) { if (v > m) m = v; };
    for (int k = 0; k < n; ++k) {
      const Blk& b = g.b[k];
      up(gb[k & 1], (uint64_t)b.M * b.cout * es), up(gb[(k + 1) & 1], (uint64_t)B * b.h * b.w * b.cin * es);
      up(gdw, (uint64_t)b.M * b.cin * es);
      if (b.blur) up(gt, (uint64_t)b.M * b.cin * es);
    }
    p.i_g[0] = bw.add(gb[0]), p.i_g[1] = bw.add(gb[1]), p.i_gdw = bw.add(gdw), p.i_gt = bw.add(gt);
    if (bc) {
      p.i_wg = bw.add(scratch_bc(p, g));
    } else {
      const ScratchFp32 sc = scratch_fp32(p, g);
      p.i_wg = bw.add(sc.wg), p.i_pw = bw.add(sc.pw), p.i_dwrows = bw.add(sc.dwrows), p.i_any = bw.add(sc.any);
    }
    p.arena_floats = Offsets(p).grad[p.nparams];
  }
  p.ws_bytes[1] = bw.cur;
  TTK_REQUIRE(!f.overflow && !bw.overflow, "mobilenet_plan_init: more than %d sub-buffers", TTK_MOBILENET_MAX_BUFFERS);
  // the launch counts, from a dry run of the sequences themselves
  const Args none;
  for (int d = 0; d < 2; ++d) {
    Seq dry{true, nullptr, 0, 0, 0};
    p.launches[d] = 0;
    if (d == 1 && p.mode == TTK_MOBILENET_EVAL) continue;
    TTK_REQUIRE(emit(p, none, dry, d) == 0, "mobilenet_plan_init: internal error in the dry run");
    p.launches[d] = dry.count;
  }
  p.check = plan_check(p);
  return 0;
}

#undef TTK_F
#undef TTK_CF
#undef TTK_SEQ_CALL
#undef TTK_SEQ_TRY
}  // namespace

extern "C" {

int ttk_mobilenet_plan_init(ttk_mobilenet_plan* plan, int B, int H, int W, int c0, int nblocks, const int* cin, const int* cout,
                            const int* stride, const int* blur, int mode, int precision, int deterministic) {
  TTK_REQUIRE(plan, "mobilenet_plan_init: plan must not be NULL");
  memset(plan, 0, sizeof(*plan));
  plan->B = B, plan->H = H, plan->W = W, plan->c0 = c0, plan->nblocks = nblocks, plan->mode = mode, plan->precision = precision,
  plan->deterministic = deterministic;
  const int rc = plan_fill(*plan, cin, cout, stride, blur);
  if (rc != 0) memset(plan, 0, sizeof(*plan));
  return rc;
}

size_t ttk_mobilenet_plan_bytes(void) { return sizeof(ttk_mobilenet_plan); }
size_t ttk_mobilenet_forward_workspace_bytes(const ttk_mobilenet_plan* plan) { return plan_ok(plan) ? (size_t)plan->ws_bytes[0] : 0; }
size_t ttk_mobilenet_backward_workspace_bytes(const ttk_mobilenet_plan* plan) { return plan_ok(plan) ? (size_t)plan->ws_bytes[1] : 0; }

int ttk_mobilenet_describe(const ttk_mobilenet_plan* plan, int backward, char* names, size_t capacity, size_t* needed) {
  TTK_REQUIRE(plan_ok(plan), "mobilenet_describe: plan was not filled by ttk_mobilenet_plan_init, or was changed after it");
  TTK_REQUIRE(!backward || plan->mode != TTK_MOBILENET_EVAL, "mobilenet_describe: backward = 1 on a plan of mode TTK_MOBILENET_EVAL (forward only)");
  const Args none;
  Seq dry{true, names, capacity, 0, 0};
  TTK_REQUIRE(emit(*plan, none, dry, backward != 0) == 0, "mobilenet_describe: internal error");
  if (needed) *needed = dry.len;
  if (!names) return dry.count;  // a size query
  TTK_REQUIRE(dry.len <= capacity, "mobilenet_describe: capacity = %zu bytes, the list takes %zu", capacity, dry.len);
  names[dry.len ? dry.len - 1 : 0] = 0;  // (the last separator becomes the terminator)
  return dry.count;
}

int ttk_mobilenet_forward(const ttk_mobilenet_plan* plan, const float* x, const float* const* params, int nparams, void* const* buffers,
                          int nbuffers, const float* const* blur_kernels, float momentum, float eps, void* workspace,
                          size_t workspace_bytes, float* feat, ttk_stream_t stream) {
  TTK_REQUIRE(plan_ok(plan), "mobilenet_forward: plan was not filled by ttk_mobilenet_plan_init, or its block table was changed after it");
  TTK_REQUIRE(x && feat, "mobilenet_forward: x and feat must not be NULL");
  TTK_REQUIRE(params && nparams == plan->nparams, "mobilenet_forward: params / nparams = %d: the plan's block table takes %d parameter tensors", nparams, plan->nparams);
  TTK_REQUIRE(buffers && nbuffers == plan->nbuffers, "mobilenet_forward: buffers / nbuffers = %d: the plan's block table takes %d BatchNorm buffers", nbuffers, plan->nbuffers);
  for (int i = 0; i < nparams; ++i) TTK_REQUIRE(params[i], "mobilenet_forward: params[%d] is NULL", i);
  for (int i = 0; i < nbuffers; ++i) TTK_REQUIRE(buffers[i] || i % 3 == 2, "mobilenet_forward: buffers[%d] is NULL (only num_batches_tracked may be)", i);
  for (int k = 0; k < plan->nblocks; ++k)
    TTK_REQUIRE(!plan->blur[k] || (blur_kernels && blur_kernels[k]), "mobilenet_forward: blur_kernels[%d] is NULL but the plan's blur mask is set there", k);
  TTK_REQUIRE(workspace && workspace_bytes >= plan->ws_bytes[0], "mobilenet_forward: workspace / workspace_bytes = %zu: the plan takes %llu", workspace_bytes, (unsigned long long)plan->ws_bytes[0]);
  TTK_REQUIRE(((uintptr_t)workspace & 255) == 0, "mobilenet_forward: workspace must be 256-byte aligned");
  TTK_REQUIRE(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "mobilenet_forward: momentum = %g, eps = %g", (double)momentum, (double)eps);
  const ttk_mobilenet_plan& p = *plan;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  // the BatchNorm constant blocks start at zero (row TTK_BN_AUX is raised with atomicMax); the blurred tensors' blocks are the identity map
  hipError_t e = hipMemsetAsync(ws + p.buf_off[0][p.i_bn], 0, p.buf_bytes[0][p.i_bn], st);
  for (int k = 0; k < p.nblocks && e == hipSuccess; ++k)
    if (p.i_idbn[k] >= 0) {
      float* id = reinterpret_cast<float*>(ws + p.buf_off[0][p.i_idbn[k]]);
      const int C = p.cin[k];
      e = hipMemsetAsync(id, 0, (size_t)TTK_BN_ROWS * C * 4, st);
      if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(id + TTK_BN_SCALE * C), 0x3f800000, C, st);
      if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(id + TTK_BN_RSTD * C), 0x3f800000, C, st);
    }
  if (e != hipSuccess) {
    ttk::set_error("mobilenet_forward: zero fill: %s", hipGetErrorString(e));
    return (int)e;
  }
  Args a;
  a.x = x, a.params = params, a.buffers = buffers, a.blur = blur_kernels, a.momentum = momentum, a.eps = eps, a.fws = ws, a.feat = feat, a.stream = stream;
  Seq run{false, nullptr, 0, 0, 0};
  return emit(p, a, run, 0);
}

int ttk_mobilenet_backward(const ttk_mobilenet_plan* plan, const float* gfeat, const float* x, const float* const* params, int nparams,
                           const float* const* blur_kernels, void* forward_workspace, size_t forward_workspace_bytes,
                           void* backward_workspace, size_t backward_workspace_bytes, float* grad_arena, size_t arena_floats,
                           ttk_mobilenet_ready_fn on_ready, void* user, ttk_stream_t stream) {
  TTK_REQUIRE(plan_ok(plan), "mobilenet_backward: plan was not filled by ttk_mobilenet_plan_init, or its block table was changed after it");
  TTK_REQUIRE(plan->mode != TTK_MOBILENET_EVAL, "mobilenet_backward: the plan's mode is TTK_MOBILENET_EVAL (forward only)");
  TTK_REQUIRE(gfeat && x, "mobilenet_backward: gfeat and x must not be NULL");
  TTK_REQUIRE(params && nparams == plan->nparams, "mobilenet_backward: params / nparams = %d: the plan's block table takes %d parameter tensors", nparams, plan->nparams);
  for (int i = 0; i < nparams; ++i) TTK_REQUIRE(params[i], "mobilenet_backward: params[%d] is NULL", i);
  for (int k = 0; k < plan->nblocks; ++k)
    TTK_REQUIRE(!plan->blur[k] || (blur_kernels && blur_kernels[k]), "mobilenet_backward: blur_kernels[%d] is NULL but the plan's blur mask is set there", k);
  TTK_REQUIRE(forward_workspace && forward_workspace_bytes >= plan->ws_bytes[0], "mobilenet_backward: forward_workspace / forward_workspace_bytes = %zu: the plan takes %llu", forward_workspace_bytes, (unsigned long long)plan->ws_bytes[0]);
  TTK_REQUIRE(backward_workspace && backward_workspace_bytes >= plan->ws_bytes[1], "mobilenet_backward: backward_workspace / backward_workspace_bytes = %zu: the plan takes %llu", backward_workspace_bytes, (unsigned long long)plan->ws_bytes[1]);
  TTK_REQUIRE((((uintptr_t)forward_workspace | (uintptr_t)backward_workspace) & 255) == 0, "mobilenet_backward: the workspaces must be 256-byte aligned");
  TTK_REQUIRE(grad_arena && arena_floats >= plan->arena_floats, "mobilenet_backward: grad_arena / arena_floats = %zu: the plan takes %llu", arena_floats, (unsigned long long)plan->arena_floats);
  const hipError_t e = hipMemsetAsync(grad_arena, 0, (size_t)plan->arena_floats * 4, (hipStream_t)stream);
  if (e != hipSuccess) {
    ttk::set_error("mobilenet_backward: zero fill: %s", hipGetErrorString(e));
    return (int)e;
  }
  Args a;
  a.x = x, a.params = params, a.blur = blur_kernels, a.fws = static_cast<char*>(forward_workspace), a.bws = static_cast<char*>(backward_workspace);
  a.gfeat = gfeat, a.arena = grad_arena, a.on_ready = on_ready, a.user = user, a.stream = stream;
  Seq run{false, nullptr, 0, 0, 0};
  return emit(*plan, a, run, 1);
}

}  // extern "C"
