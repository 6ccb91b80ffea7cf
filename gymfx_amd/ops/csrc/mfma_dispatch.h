// Tile dispatch of the MFMA GEMM and wgrad launchers as pure host functions:
// (shape, flags, knob values) -> which kernel instantiation runs on what
// grid.  launch_gemm / launch_wgrad (ppo_kernels.hip) call these with the
// process-wide knob values; the gemm_variant / wgrad_variant bindings call
// them with any knob values, so a test can ask "what would be launched"
// without touching the GPU.  Plain C++ (no HIP), so it also compiles into a
// stand-alone host program.
//
// The X-macro lists below are the ONLY place an instantiation is named: the
// launchers expand them into their dispatch chains (which instantiates the
// kernels) and mfma_variant_names() expands them into the list the tests
// must cover.  A combination select_*() can return that is not in the list
// has no kernel: the launcher aborts and the binding raises.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace gymfx {

// Knob values: -1 = unset (the heuristic decides), otherwise the integer
// the environment variable holds.
struct GemmKnobs {
  int wide = -1;  // GYMFX_GEMM_WIDE: 1 forces 64x256 tiles, 4 forces 64x128
  int bk64 = -1;  // GYMFX_GEMM_BK64: 1 forces the BK=64 pipeline, 0 off
  int n1 = -1;    // GYMFX_GEMM_N1: 1 forces the 64x32 tile, 0 off
};

inline int knob_from_env(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : -1;
}

// read once per process, like every other knob of the extension
inline const GemmKnobs& process_gemm_knobs() {
  static const GemmKnobs k = [] {
    GemmKnobs v;
    v.wide = knob_from_env("GYMFX_GEMM_WIDE");
    v.bk64 = knob_from_env("GYMFX_GEMM_BK64");
    v.n1 = knob_from_env("GYMFX_GEMM_N1");
    return v;
  }();
  return k;
}

inline int process_wgrad_big_knob() {
  static const int big = knob_from_env("GYMFX_WGRAD_BIG");
  return big;
}

inline int dispatch_ceil_div(int a, int b) { return (a + b - 1) / b; }

// gemm_kernel<TB, ACT, DT, AB, NF, ACC, BK, PERM> on a (gx, gy) grid
struct GemmSel {
  bool tb;
  int act;
  bool dt, ab;
  int nf;
  bool acc;
  int bk;
  bool perm;
  int gx, gy;
};

inline GemmSel select_gemm(int M, int N, int K, bool trans_b, int act,
                           bool dact_tanh, bool add_bias, bool accum,
                           bool a_perm, const GemmKnobs& kn) {
  // Tile width: 64x64 (NFRAG=2) tiles run at occupancy 8 and beat the
  // 64x256 (NFRAG=8, occupancy 3) wide tiles even at tall update shapes
  // (M=65536: 20.3 vs 22.0 ms/update whole-trainer) — the extra occupancy
  // hides HBM latency better than wide tiles save A-operand re-streaming
  // (L2 absorbs the re-reads).  GYMFX_GEMM_WIDE=1 forces the wide tile,
  // =4 the 64x128 middle tile (tuning knobs).
  // Tile-width heuristic: at N >= 1024 the 64-wide tile re-streams the A
  // operand N/64 times (the LSTM Wx gates GEMM read its 34 MB A slab 16x
  // = 544 MB/call); the 64x128 tile halves that and wins big there.
  // The round-1 "wide loses" measurement holds only for N <= 256 outputs.
  const bool mid = (N >= 96) &&
                   (kn.wide == 4 ||
                    (kn.wide == -1 && N >= 1024 && M >= 16384));
  const bool wide = (N >= 192) && !mid && kn.wide == 1;
  // BK=64 staging pipeline (half the barriers) for long-K trans_b shapes —
  // ROADMAP lever 2.  measured: BK=64 wins for long-K shapes (LSTM dgates
  // dgrad K=1024: update 41.5 -> 39.9 ms) and LOSES at K<=260 (MLP headline
  // 28.4 -> 27.4M) — auto-enable only at K >= 512
  const bool bk64 = trans_b && !wide && !mid &&
                    (kn.bk64 == 1 || (kn.bk64 != 0 && K >= 512));
  const int gx = dispatch_ceil_div(M, 64);
  // Narrow 64x32 tile (NFRAG=1, BK=64 only — see the BLPT static_assert):
  // at N=256 the 64x64 tile fills exactly 1 block/CU (the LSTM bwd-chain
  // dgrad: 64x4 = 256 workgroups) while occupancy allows more; BN=32
  // doubles the grid for latency hiding at 2x B re-streaming.
  // GYMFX_GEMM_N1=1 forces on, =0 off, unset = auto (M*N small, long K).
  if (bk64 && act == 0 && !dact_tanh && !add_bias && !accum && !a_perm &&
      N <= 256 &&
      (kn.n1 == 1 || (kn.n1 == -1 && (int64_t)M * N <= 64 * 64 * 256)))
    return {true, 0, false, false, 1, false, 64, false, gx,
            dispatch_ceil_div(N, 32)};
  if (a_perm) {
    // gather+first-GEMM fusion: only the L1 forward combo is instantiated
    // (trans_b, tanh epilogue, bias, 64x64 tile), so the grid is sized for
    // THAT tile whatever wide/mid say — a grid sized for a 128- or 256-wide
    // tile left the columns past the first 64 of every tile unwritten.
    // Any other flag combination is passed through as asked and has no
    // kernel (models/mlp.py passes a_feistel only on the first layer).
    const int a = act == 0 ? 0 : (act == 1 ? 1 : 2);
    return {trans_b, a, dact_tanh, add_bias, 2, accum, 32, true, gx,
            dispatch_ceil_div(N, 64)};
  }
  const int nf = wide ? 8 : (mid ? 4 : 2);
  const int gy = dispatch_ceil_div(N, 32 * nf);
  // C += A@B (f32 out, no bias/activation): the LSTM recurrent GEMM
  if (accum) return {trans_b, 0, false, false, nf, true, 32, false, gx, gy};
  const int bk = (nf == 2 && bk64) ? 64 : 32;
  // tanh' dgrad epilogue: bf16 out, no bias
  if (dact_tanh) return {trans_b, 1, true, false, nf, false, bk, false, gx, gy};
  const int a = act == 0 ? 0 : (act == 1 ? 1 : 2);
  return {trans_b, a, false, add_bias, nf, false, bk, false, gx, gy};
}

// X(TB, ACT, DT, AB, NF, ACC, BK, PERM): the seven epilogues of one tile
#define GYMFX_GEMM_EPILOGUES(X, TB, NF, BK)                                   \
  X(TB, 0, false, false, NF, false, BK, false)                                \
  X(TB, 0, false, true, NF, false, BK, false)                                 \
  X(TB, 1, false, false, NF, false, BK, false)                                \
  X(TB, 1, false, true, NF, false, BK, false)                                 \
  X(TB, 2, false, false, NF, false, BK, false)                                \
  X(TB, 2, false, true, NF, false, BK, false)                                 \
  X(TB, 1, true, false, NF, false, BK, false)

#define GYMFX_GEMM_VARIANTS(X)                                                \
  GYMFX_GEMM_EPILOGUES(X, true, 2, 32)                                        \
  GYMFX_GEMM_EPILOGUES(X, true, 2, 64)                                        \
  GYMFX_GEMM_EPILOGUES(X, true, 4, 32)                                        \
  GYMFX_GEMM_EPILOGUES(X, true, 8, 32)                                        \
  GYMFX_GEMM_EPILOGUES(X, false, 2, 32)                                       \
  GYMFX_GEMM_EPILOGUES(X, false, 4, 32)                                       \
  GYMFX_GEMM_EPILOGUES(X, false, 8, 32)                                       \
  X(true, 0, false, false, 2, true, 32, false)                                \
  X(true, 0, false, false, 4, true, 32, false)                                \
  X(true, 0, false, false, 8, true, 32, false)                                \
  X(false, 0, false, false, 2, true, 32, false)                               \
  X(false, 0, false, false, 4, true, 32, false)                               \
  X(false, 0, false, false, 8, true, 32, false)                               \
  X(true, 0, false, false, 1, false, 64, false)                               \
  X(true, 2, false, true, 2, false, 32, true)

inline bool gemm_sel_is(const GemmSel& s, bool tb, int act, bool dt, bool ab,
                        int nf, bool acc, int bk, bool perm) {
  return s.tb == tb && s.act == act && s.dt == dt && s.ab == ab &&
         s.nf == nf && s.acc == acc && s.bk == bk && s.perm == perm;
}

inline std::string gemm_name(bool tb, int act, bool dt, bool ab, int nf,
                             bool acc, int bk, bool perm) {
  char buf[96];
  snprintf(buf, sizeof buf, "tb%d_act%d_dt%d_ab%d_nf%d_bk%d_acc%d_perm%d",
           (int)tb, act, (int)dt, (int)ab, nf, bk, (int)acc, (int)perm);
  return buf;
}

inline std::string gemm_name(const GemmSel& s) {
  return gemm_name(s.tb, s.act, s.dt, s.ab, s.nf, s.acc, s.bk, s.perm);
}

inline bool gemm_instantiated(const GemmSel& s) {
#define GYMFX_X(TB, ACT, DT, AB, NF, ACC, BK, PERM)                           \
  if (gemm_sel_is(s, TB, ACT, DT, AB, NF, ACC, BK, PERM)) return true;
  GYMFX_GEMM_VARIANTS(GYMFX_X)
#undef GYMFX_X
  return false;
}

// Weight-resident tall GEMM (gemm_resident_kernel): a separate entry point
// beside select_gemm, which it never changes.  The whole [256, K] weight
// matrix sits in one LDS image per workgroup.
constexpr int RESIDENT_N = 256;      // output columns, exactly
constexpr int RESIDENT_LD = 264;     // LDS row stride in elements = max K
constexpr int RESIDENT_GROUP = 256;  // rows of A per workgroup iteration

// Structural only: the shape and epilogue the kernel implements.  Any M >= 1
// is accepted (the kernel guards a ragged last group).  K % 4 == 0 because
// rows are read in 8-byte pieces.  Whether the kernel is FASTER at a given M
// is the caller's call (ActorCriticMLP.resident_min_rows).
inline bool gemm_resident_ok(int64_t M, int64_t N, int64_t K, bool trans_b,
                             int act, bool dact_tanh, bool add_bias,
                             bool accum, bool a_perm = false) {
  if (M < 1 || M > INT32_MAX - RESIDENT_GROUP) return false;
  if (N != RESIDENT_N || K < 4 || K > RESIDENT_LD || K % 4 != 0) return false;
  if (!trans_b || accum || a_perm) return false;
  const bool fwd = act == 2 && add_bias && !dact_tanh;   // bias + tanh
  const bool dgrad = act == 1 && dact_tanh && !add_bias;  // x (1 - y^2)
  return fwd || dgrad;
}

// workgroups: one per 256-row group up to the CU count (or the caller's cap)
inline int gemm_resident_grid(int64_t M, int n_cus, int max_blocks) {
  const int64_t groups = (M + RESIDENT_GROUP - 1) / RESIDENT_GROUP;
  int64_t cap = max_blocks > 0 ? max_blocks : n_cus;
  if (cap < 1) cap = 1;
  return (int)(groups < cap ? groups : cap);
}

// wgrad_glds_kernel / wgrad_partial_kernel <DB, FK, FN, PERM> on (gx,gy,gz)
struct WgradSel {
  bool glds;
  bool db;
  int fk, fn;
  bool perm;
  int gx, gy, gz;
};

inline WgradSel select_wgrad(int M, int N, int K, int slabs, bool want_db,
                             bool x_perm, int big_knob) {
  // Tile choice: 128x128 halves the HBM re-streaming of X/dY — wgrad runs
  // at ~5.7 TB/s with 64x64 tiles, i.e. bandwidth-bound, so the bigger tile
  // wins whenever the grid still fills the chip (MLP 260x256 shapes:
  // 19.3 -> 18.5 ms/update whole-trainer).  384+ workgroups = 1.5 waves/SIMD
  // at the kernel's occupancy 2 keeps every CU fed.
  // GYMFX_WGRAD_BIG=0/1 overrides (tuning knob).
  const bool big =
      K >= 128 && N >= 128 &&
      (big_knob >= 0 ? big_knob != 0
                     : (int64_t)dispatch_ceil_div(K, 128) *
                               dispatch_ceil_div(N, 128) * slabs >=
                           384);
  const int m_per_slab = (M + slabs - 1) / slabs;
  // glds path (both tile configs): full N tiles and full 64-row m-chunks
  // only; everything else runs the register-staged kernel.
  const int TW = big ? 128 : 64;
  const bool glds_ok =
      N % TW == 0 && K >= TW && m_per_slab % 64 == 0 && M % slabs == 0;
  if (glds_ok) {
    // the glds kernel masks a partial final K tile in-kernel (guarded
    // register staging + grow<K epilogue guard), so NO separate tail pass
    // over dY is needed.  For K=260 the 5x4 tile (TK=160) covers K in TWO
    // passes where 128-wide tiles need three — one fewer full dY read
    // (~1.5 ms/update on the LSTM wgrads).
    if (big) {
      // 5x4 (TK=160) saves a dY pass for K=260 but its 80-VGPR accs spill
      // at N >= 1024 (LSTM Wx wgrad measured 187 us vs 144 for 4x4+tail)
      const int t44 = dispatch_ceil_div(K, 128);
      const int t54 = dispatch_ceil_div(K, 160);
      if (t54 < t44 && N <= 512)
        return {true, want_db, 5, 4, x_perm, t54, N / TW, slabs};
      return {true, want_db, 4, 4, x_perm, t44, N / TW, slabs};
    }
    return {true, want_db, 2, 2, x_perm, dispatch_ceil_div(K, 64), N / TW,
            slabs};
  }
  const int f = big ? 4 : 2;
  return {false, want_db, f, f, x_perm, dispatch_ceil_div(K, 32 * f),
          dispatch_ceil_div(N, 32 * f), slabs};
}

// X(DB, FK, FN, PERM)
#define GYMFX_WGRAD_TILE(X, FK, FN)                                           \
  X(true, FK, FN, false)                                                      \
  X(false, FK, FN, false)                                                     \
  X(true, FK, FN, true)                                                       \
  X(false, FK, FN, true)

#define GYMFX_WGRAD_GLDS_VARIANTS(X)                                          \
  GYMFX_WGRAD_TILE(X, 2, 2)                                                   \
  GYMFX_WGRAD_TILE(X, 4, 4)                                                   \
  GYMFX_WGRAD_TILE(X, 5, 4)

#define GYMFX_WGRAD_PARTIAL_VARIANTS(X)                                       \
  GYMFX_WGRAD_TILE(X, 2, 2)                                                   \
  GYMFX_WGRAD_TILE(X, 4, 4)

inline bool wgrad_sel_is(const WgradSel& s, bool glds, bool db, int fk, int fn,
                         bool perm) {
  return s.glds == glds && s.db == db && s.fk == fk && s.fn == fn &&
         s.perm == perm;
}

inline std::string wgrad_name(bool glds, bool db, int fk, int fn, bool perm) {
  char buf[64];
  snprintf(buf, sizeof buf, "%s_db%d_%dx%d_perm%d", glds ? "glds" : "partial",
           (int)db, fk, fn, (int)perm);
  return buf;
}

inline std::string wgrad_name(const WgradSel& s) {
  return wgrad_name(s.glds, s.db, s.fk, s.fn, s.perm);
}

// every instantiated gemm_kernel / wgrad_glds_kernel / wgrad_partial_kernel
inline std::vector<std::string> mfma_variant_names() {
  std::vector<std::string> v;
#define GYMFX_X(TB, ACT, DT, AB, NF, ACC, BK, PERM)                           \
  v.push_back(gemm_name(TB, ACT, DT, AB, NF, ACC, BK, PERM));
  GYMFX_GEMM_VARIANTS(GYMFX_X)
#undef GYMFX_X
#define GYMFX_X(DB, FK, FN, PERM) v.push_back(wgrad_name(true, DB, FK, FN, PERM));
  GYMFX_WGRAD_GLDS_VARIANTS(GYMFX_X)
#undef GYMFX_X
#define GYMFX_X(DB, FK, FN, PERM) v.push_back(wgrad_name(false, DB, FK, FN, PERM));
  GYMFX_WGRAD_PARTIAL_VARIANTS(GYMFX_X)
#undef GYMFX_X
  return v;
}

}  // namespace gymfx
