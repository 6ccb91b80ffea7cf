// PPO compute stack for gfx950 (CDNA4): hand-written MFMA bf16 GEMMs with
// fused epilogues (bias+tanh fwd, tanh' dgrad), deterministic split-M wgrad,
// GAE backward scan, fused Adam, categorical sampling with counter-based RNG,
// and the PPO clipped-surrogate loss backward.
//
// The reference is agent-free by design (/root/reference/app/env.py:148-150);
// this stack is the BASELINE.json north-star requirement (PPO MLP(256,256)
// bf16 on MFMA, GAE scan, minibatch Adam).
//
// MFMA: v_mfma_f32_16x16x32_bf16 — per-wave 16x16 tile, K=32, fp32 accum.
// Lane mapping (cdna_hip_programming.md §3):
//   A: lane l holds A[row = l&15][k = (l>>4)*8 + i], i=0..7  (8 bf16)
//   B: lane l holds B[k = (l>>4)*8 + i][col = l&15]
//   C/D: lane l, reg r -> row = (l>>4)*4 + r, col = l&15
// Verified on hardware by tests/test_gpu_gemm.py (identity x asymmetric-B
// probes per guide rule G9).
#include "env_common.h"
#include "mfma_dispatch.h"

#include <hip/hip_bf16.h>

#include <algorithm>

namespace gymfx {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

GFX_DEV float bf2f(__bf16 v) { return (float)v; }
GFX_DEV __bf16 f2bf(float v) { return (__bf16)v; }

// Inline tanh via the hardware exp (v_exp_f32).  libm tanhf is an actual
// CALL on gfx950: inside the GEMM epilogue it forced every live MFMA
// accumulator to scratch (272 B/thread of spill, 6x slowdown).  Accuracy is
// ~2 ulp of fp32 — far below the bf16 output rounding.
// fast_exp/fast_log/splitmix64 live in env_common.h (shared with the fused
// env_step sampling path so every sampler implementation agrees bitwise).
GFX_DEV float fast_tanh(float x) {
  x = fminf(fmaxf(x, -15.f), 15.f);
  // raw v_exp_f32 + v_rcp_f32, both single instructions.  An IEEE f32
  // divide here expands to a ~10-op guarded Newton sequence; unrolled 64x
  // in the wide epilogue that blew register pressure enough to demote the
  // MFMA accumulators to scratch for the whole kernel.
  const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// The two update-phase GEMM epilogues, shared by gemm_kernel and
// gemm_resident_kernel so both contract the same way (bitwise equal bf16).
GFX_DEV float epi_bias_tanh(float v, float b) { return fast_tanh(v + b); }
GFX_DEV float epi_dtanh(float v, __bf16 yact) {
  const float y = bf2f(yact);
  return v * (1.f - y * y);
}

GFX_DEV uint32_t feistel_encrypt_once(uint32_t x, int half, uint32_t mask,
                                      uint64_t key) {
  uint32_t a = x & mask;        // low half
  uint32_t b = x >> half;       // high half
  for (int r = 0; r < 4; ++r) {
    const uint32_t f =
        (uint32_t)(splitmix64(key ^ ((uint64_t)r << 48) ^ (uint64_t)b)) & mask;
    const uint32_t t = b;
    b = a ^ f;
    a = t;
  }
  return (b << half) | a;
}

GFX_DEV uint32_t feistel_perm_idx(uint32_t i, uint32_t n, int half,
                                  uint64_t key) {
  const uint32_t mask = (1u << half) - 1u;
  uint32_t x = i;
  do {
    x = feistel_encrypt_once(x, half, mask, key);
  } while (x >= n);  // cycle-walk: terminates (bijection over 2^(2*half))
  return x;
}

// Row indirection for the gather+first-GEMM fusion: the L1 forward GEMM
// (and the W1 wgrad) read the rollout slab obs_flat THROUGH the epoch
// permutation instead of a materialized obs_mb copy (ROADMAP lever 3 —
// saves one full write+read pass over the minibatch observations).
// ctr_off: the gather that produced the OTHER minibatch fields has already
// advanced mb_ctr when these kernels run (-1 in the trainer's sequence).
// (FeistelMap struct lives in env_common.h — host code builds it.)
GFX_DEV uint64_t feistel_key(const FeistelMap& fm, uint32_t* mb) {
  const unsigned long long ctr =
      (unsigned long long)((long long)*fm.mb_ctr + fm.ctr_off);
  const uint32_t epoch = (uint32_t)(ctr / (unsigned)fm.minibatches);
  *mb = (uint32_t)(ctr % (unsigned)fm.minibatches);
  return splitmix64(fm.seed ^ (*fm.step_base * 0x9E3779B97F4A7C15ull) ^
                    ((uint64_t)epoch << 32));
}

GFX_DEV int64_t feistel_src_row(const FeistelMap& fm, uint64_t key,
                                uint32_t mb, int row) {
  return (int64_t)feistel_perm_idx(mb * (uint32_t)fm.M_mb + (uint32_t)row,
                                   fm.n, fm.half, key);
}

// ---------------------------------------------------------------------------
// GEMM: C[M,N] = act(A[M,K] @ B + bias)
//   TRANS_B = false: B stored [K, N] (ldb = N)
//   TRANS_B = true:  B stored [N, K] (ldb = K)  (used for dgrad: B = W^T)
// Block: 256 threads = 4 waves in a 2x2 wave grid; BK = 32; double-buffered
// LDS staging (global loads for tile k+1 issue in registers while MFMAs for
// tile k run — one __syncthreads per K-step).
// NFRAG = MFMA n-fragments per wave:
//   NFRAG=2 -> block tile 64x64  (the DEFAULT at every shape: occupancy 8
//              hides memory latency better than wider tiles save A-operand
//              re-streaming — L2 absorbs the re-reads; see launch_gemm)
//   NFRAG=4/8 -> 64x128 / 64x256 tiles, reachable via GYMFX_GEMM_WIDE
//              (measured slower: occupancy 2-3, 67% SQ_WAIT)
// Epilogues: ACT 0=none(f32 out) 1=none(bf16) 2=tanh(bf16)
//            DACT_TANH: multiply by (1 - Y^2) elementwise (dgrad fused tanh')
// ---------------------------------------------------------------------------
// min-waves floor 2: with the tanh epilogue the allocator otherwise chases
// a higher occupancy target and demotes the 64 MFMA accumulators of the
// NFRAG=8 variant to scratch — 1.2 GB of per-call scratch traffic, 4x
// slower than just running 2 waves/SIMD with accs in AGPRs.
// BKT: K-chunk depth of the LDS staging pipeline.  32 is the default; 64
// halves the barrier count for long-K tall shapes (the dgrad/fwd GEMMs of
// the update phase are latency-limited at 32 — ROADMAP lever 2), reachable
// via GYMFX_GEMM_BK64.  The MFMA k order is unchanged (two sequential
// 16x16x32 steps per 64-chunk), so results stay bitwise identical.
template <bool TRANS_B, int ACT, bool DACT_TANH, bool ADD_BIAS, int NFRAG,
          bool ACCUM = false, int BKT = 32, bool A_PERM = false>
__global__ __launch_bounds__(256, 2) void gemm_kernel(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    const float* __restrict__ bias, void* __restrict__ C,
    const __bf16* __restrict__ Yact,  // activation output (DACT_TANH)
    int M, int N, int K, FeistelMap fm = FeistelMap{}) {
  constexpr int BM = 64, BK = BKT;
  constexpr int BN = 32 * NFRAG;
  // TRANS_B images are UNPADDED linear (required by the glds staging; the
  // b128 fragment-read bank multiplicity is already at its minimum for both
  // strides).  !TRANS_B keeps the +8 pad with register staging.
  constexpr int LDA = TRANS_B ? BK : (BK + 8);
  // B tile layout follows the GLOBAL layout so staging loads are always
  // contiguous bf16x8 (a strided 2-byte gather of B was 6x slower than the
  // whole GEMM): TRANS_B stages [n][k], !TRANS_B stages [k][n]; the
  // !TRANS_B fragment reads transpose out of LDS instead.
  constexpr int BS_ROWS = TRANS_B ? BN : BK;
  constexpr int BS_LD = TRANS_B ? BK : (BN + 8);
  __shared__ __align__(16) __bf16 As[2][BM][LDA];
  __shared__ __align__(16) __bf16 Bs[2][BS_ROWS][BS_LD];

  const int bm = blockIdx.x * BM;
  const int bn = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;         // 0..3
  const int lane = tid & 63;
  const int wr = wave >> 1;          // wave row 0..1
  const int wc = wave & 1;           // wave col 0..1

  f32x4 acc[2][NFRAG] = {};

  // gather+first-GEMM fusion: A rows go through the epoch permutation
  uint64_t fkey = 0;
  uint32_t fmb = 0;
  if (A_PERM) fkey = feistel_key(fm, &fmb);
  auto a_row = [&](int gr) -> int64_t {
    return A_PERM ? feistel_src_row(fm, fkey, fmb, gr) : (int64_t)gr;
  };

  const int row_a = lane & 15;
  const int kseg = lane >> 4;  // 0..3 -> k-base = kseg*8

  // staging: element-offset addressed so any BKT works; for BKT=32 the
  // (row, col) decomposition reduces to the classic tid>>2 / (tid&3)*8
  constexpr int ALPT = (BM * BK) / 2048;  // bf16x8 loads per thread, A tile
  constexpr int BLPT = (BN * BK) / 2048;  // bf16x8 loads per thread, B tile
  // NFRAG=1 (BN=32) tiles need BKT=64 so every thread still stages >=1
  // bf16x8 of B (32*32/2048 would truncate to 0 loads)
  static_assert(ALPT >= 1 && BLPT >= 1, "tile too small for 256-thread staging");

  bf16x8 ra[ALPT], rb[BLPT];

  auto load_tile = [&](int k0) {
    // A tile [BM m][BK k]
    for (int j = 0; j < ALPT; ++j) {
      ra[j] = bf16x8{};
      const int e = (tid + j * 256) * 8;
      const int gr = bm + e / BK;
      if (gr < M) {
        const int64_t sr = a_row(gr);
        const int gk = k0 + e % BK;
        if (gk + 8 <= K) {
          ra[j] = *reinterpret_cast<const bf16x8*>(&A[sr * K + gk]);
        } else {
          for (int i = 0; i < 8; ++i)
            ra[j][i] = (gk + i < K) ? A[sr * K + gk + i] : (__bf16)0.f;
        }
      }
    }
    if (TRANS_B) {
      // stage [n][k]: contiguous along k in global [N, K]
      for (int j = 0; j < BLPT; ++j) {
        rb[j] = bf16x8{};
        const int e = (tid + j * 256) * 8;
        const int gn = bn + e / BK;
        if (gn < N) {
          const int gk = k0 + e % BK;
          if (gk + 8 <= K) {
            rb[j] = *reinterpret_cast<const bf16x8*>(&B[(int64_t)gn * K + gk]);
          } else {
            for (int i = 0; i < 8; ++i)
              rb[j][i] = (gk + i < K) ? B[(int64_t)gn * K + gk + i] : (__bf16)0.f;
          }
        }
      }
    } else {
      // stage [k][n]: contiguous along n in global [K, N]
      for (int j = 0; j < BLPT; ++j) {
        rb[j] = bf16x8{};
        const int c = tid + j * 256;             // chunk over [BK][BN/8]
        const int kk = c / (BN / 8);
        const int n8 = (c % (BN / 8)) * 8;
        const int gk = k0 + kk;
        const int gn = bn + n8;
        if (gk < K) {
          if (gn + 8 <= N) {
            rb[j] = *reinterpret_cast<const bf16x8*>(&B[(int64_t)gk * N + gn]);
          } else {
            for (int i = 0; i < 8; ++i)
              rb[j][i] = (gn + i < N) ? B[(int64_t)gk * N + gn + i] : (__bf16)0.f;
          }
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
    for (int j = 0; j < ALPT; ++j) {
      const int e = (tid + j * 256) * 8;
      *reinterpret_cast<bf16x8*>(&As[buf][e / BK][e % BK]) = ra[j];
    }
    if (TRANS_B) {
      for (int j = 0; j < BLPT; ++j) {
        const int e = (tid + j * 256) * 8;
        *reinterpret_cast<bf16x8*>(&Bs[buf][e / BK][e % BK]) = rb[j];
      }
    } else {
      for (int j = 0; j < BLPT; ++j) {
        const int c = tid + j * 256;
        *reinterpret_cast<bf16x8*>(
            &Bs[buf][c / (BN / 8)][(c % (BN / 8)) * 8]) = rb[j];
      }
    }
  };

  const int ktiles = (K + BK - 1) / BK;
  // glds staging (TRANS_B, in-bounds blocks, full k-chunks): 16B per lane
  // into the linear images — no staging registers, loads still in flight
  // across the MFMA section and drained by the barrier's vmcnt(0).
  const bool can_glds = TRANS_B && (bm + BM <= M) && (bn + BN <= N);
  auto glds_tile = [&](int buf, int k0) {
    for (int j = 0; j < ALPT; ++j) {  // A tile [BM][BK]
      const int e0 = (wave * ALPT + j) * 512;
      const int row = (e0 + lane * 8) / BK;
      const int col = (e0 + lane * 8) % BK;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &A[a_row(bm + row) * K + k0 + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &As[buf][0][0] + e0),
          16, 0, 0);
    }
    for (int j = 0; j < BLPT; ++j) {  // B tile [BN][BK]
      const int e0 = (wave * BLPT + j) * 512;
      const int row = (e0 + lane * 8) / BK;
      const int col = (e0 + lane * 8) % BK;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &B[(int64_t)(bn + row) * K + k0 + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &Bs[buf][0][0] + e0),
          16, 0, 0);
    }
  };
  auto stage = [&](int buf, int k0) {
    if (can_glds && k0 + BK <= K) {
      glds_tile(buf, k0);
    } else {
      load_tile(k0);
      store_tile(buf);
    }
  };

  stage(0, 0);
  __syncthreads();

  for (int kt = 0; kt < ktiles; ++kt) {
    const int cur = kt & 1;
    const bool nxt_glds =
        kt + 1 < ktiles && can_glds && (kt + 1) * BK + BK <= K;
    if (nxt_glds) glds_tile(1 - cur, (kt + 1) * BK);
    else if (kt + 1 < ktiles) load_tile((kt + 1) * BK);

    for (int ks = 0; ks < BK / 32; ++ks) {  // sequential k order: bitwise
      bf16x8 af[2], bf[NFRAG];              // identical for any BKT
      for (int mi = 0; mi < 2; ++mi)
        af[mi] = *reinterpret_cast<const bf16x8*>(
            &As[cur][wr * 32 + mi * 16 + row_a][ks * 32 + kseg * 8]);
      if (TRANS_B) {
        for (int ni = 0; ni < NFRAG; ++ni)
          bf[ni] = *reinterpret_cast<const bf16x8*>(
              &Bs[cur][wc * (16 * NFRAG) + ni * 16 + row_a][ks * 32 + kseg * 8]);
      } else {
        // transpose at the LDS read: Bs holds [k][n]
        for (int ni = 0; ni < NFRAG; ++ni)
          for (int i = 0; i < 8; ++i)
            bf[ni][i] = Bs[cur][ks * 32 + kseg * 8 + i]
                          [wc * (16 * NFRAG) + ni * 16 + row_a];
      }
      for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < NFRAG; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    }

    if (kt + 1 < ktiles && !nxt_glds) store_tile(1 - cur);
    __syncthreads();
  }

  // ---- epilogue -------------------------------------------------------
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  for (int mi = 0; mi < 2; ++mi) {
    for (int ni = 0; ni < NFRAG; ++ni) {
      const int gcol = bn + wc * (16 * NFRAG) + ni * 16 + ccol;
      if (gcol >= N) continue;
      for (int r = 0; r < 4; ++r) {
        const int grow = bm + wr * 32 + mi * 16 + crow_base + r;
        if (grow >= M) continue;
        float v = acc[mi][ni][r];
        if (ADD_BIAS && ACT == 2) {
          v = epi_bias_tanh(v, bias[gcol]);
        } else {
          if (ADD_BIAS) v += bias[gcol];
          if (ACT == 2) v = fast_tanh(v);
        }
        if (DACT_TANH) v = epi_dtanh(v, Yact[(int64_t)grow * N + gcol]);
        if (ACT == 0) {
          float* cp = reinterpret_cast<float*>(C) + (int64_t)grow * N + gcol;
          *cp = ACCUM ? (*cp + v) : v;
        } else {
          reinterpret_cast<__bf16*>(C)[(int64_t)grow * N + gcol] = f2bf(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Weight-resident tall GEMM: C[M,256] = epilogue(A[M,K] @ Wt[256,K]^T) for
// the update-phase layers (N = 256, K <= 264, M huge).  The whole weight
// matrix sits in ONE LDS image per workgroup (256 rows x 264-element stride
// = 135,168 B, K zero-padded to a multiple of 8), filled once; the
// workgroup then loops over 256-row groups of A with no barrier.  Each of
// the 8 waves owns 32 rows x 256 columns (128 f32 accumulators per lane),
// loads its A fragments straight from global into registers (every byte of
// A read exactly once) and reads the weight fragments from the image.
// gemm_kernel stages A 4x and the weights M/64 times for the same shape.
//
// Bitwise equal to gemm_kernel: same MFMA, same sequential 32-deep k chunks
// into one accumulator per output element, same zero-filled tail chunk, same
// epilogue helpers.  The MFMA runs TRANSPOSED (weights as the A operand,
// activations as B): a lane then holds 4 consecutive output COLUMNS of one
// row, so the epilogue moves 8-byte bf16x4 / 16-byte bias vectors instead
// of 2-byte scalars.  An output element depends only on its products, their
// k positions and the accumulator, not on which operand carried which.
//
// EPI 0: bias + tanh -> bf16 (act=2, forward)
// EPI 1: x (1 - Yact^2) -> bf16 (act=1 + dact_tanh, dgrad)
// NFULL_CT: number of full 32-deep k chunks when known at compile time (8 =
// the two workload shapes K=256/260: all A chunks of a pass are issued up
// front), -1 = runtime loop with a one-chunk prefetch (any K % 4 == 0).
// TAIL_CT: with NFULL_CT >= 0, whether K has a partial last chunk (behind a
// runtime test the compiler sinks the tail loads below all the MFMAs).
// ---------------------------------------------------------------------------
template <int EPI, int NFULL_CT, bool TAIL_CT = false>
__global__ __launch_bounds__(512) void gemm_resident_kernel(
    const __bf16* __restrict__ A, const __bf16* __restrict__ Wt,
    const float* __restrict__ bias, __bf16* __restrict__ C,
    const __bf16* __restrict__ Yact, int M, int K) {
  constexpr int N = RESIDENT_N, LD = RESIDENT_LD, GROUP = RESIDENT_GROUP;
  // ONE array: the weight image, then the 256 f32 biases (an epilogue that
  // loads them from global waits on vmcnt, i.e. on its own earlier stores)
  __shared__ __align__(16) __bf16 Ws[N * LD + 2 * N];
  float* bias_s = reinterpret_cast<float*>(&Ws[N * LD]);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int row_l = lane & 15;
  const int kseg = lane >> 4;  // 0..3 -> k-base = kseg*8

  const int nfull = NFULL_CT >= 0 ? NFULL_CT : K / 32;
  // 0..28, multiple of 4 (a compile-time flag in the unrolled kernels)
  const int ktail = NFULL_CT >= 0 ? (int)TAIL_CT : K - nfull * 32;
  const int kpad8 = (K + 7) & ~7;

  // tail chunk (k >= nfull*32): each lane's 8 elements as two 8-byte halves,
  // out-of-range halves read the row start and are selected to zero
  const int kt = nfull * 32 + kseg * 8;
  const bool t_lo = kt + 4 <= K, t_hi = kt + 8 <= K;
  const int t_lo_off = t_lo ? kt : 0, t_hi_off = t_hi ? kt + 4 : 0;
  const bool w_tv = kt < kpad8;  // weight image holds zeros in [K, kpad8)
  const int w_t_off = w_tv ? kt : 0;

  const __bf16* pa[2];
  auto set_rows = [&](int g) {
    for (int mi = 0; mi < 2; ++mi) {
      const int r = min(g * GROUP + wave * 32 + mi * 16 + row_l, M - 1);
      pa[mi] = A + (int64_t)r * K;
    }
  };
  auto load_full = [&](int mi, int kc) {
    return *reinterpret_cast<const bf16x8*>(pa[mi] + kc * 32 + kseg * 8);
  };
  auto load_tail = [&](int mi) {
    bf16x4 lo = *reinterpret_cast<const bf16x4*>(pa[mi] + t_lo_off);
    bf16x4 hi = *reinterpret_cast<const bf16x4*>(pa[mi] + t_hi_off);
    if (!t_lo) lo = bf16x4{};
    if (!t_hi) hi = bf16x4{};
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  };

  constexpr int LATE = (NFULL_CT >= 4 && TAIL_CT) ? 2 : 0;
  constexpr int NA = NFULL_CT >= 0 ? (NFULL_CT > 0 ? NFULL_CT : 1) : 1;
  bf16x8 a[NA][2];
  bf16x8 atail[2];
  auto load_group = [&](int g) {
    set_rows(g);
    if (NFULL_CT >= 0) {
      // with a tail the last LATE full chunks and the tail are issued as
      // the first chunks are consumed: 9 chunks live at once spill
      for (int kc = 0; kc < NFULL_CT - LATE; ++kc)
        for (int mi = 0; mi < 2; ++mi) a[kc][mi] = load_full(mi, kc);
    } else if (nfull > 0) {
      for (int mi = 0; mi < 2; ++mi) a[0][mi] = load_full(mi, 0);
    }
    // unconditional (a branch around a load costs a vmcnt(0)): with no tail
    // both halves read the row start and are selected to zero.  The unrolled
    // kernel issues these after its first chunk instead, when registers free.
    if (NFULL_CT < 0)
      for (int mi = 0; mi < 2; ++mi) atail[mi] = load_tail(mi);
  };

  // the first group's A loads fly under the weight fill
  load_group(blockIdx.x);

  {
    // All loads of the fill are issued before the first LDS write: a
    // load -> wait -> write loop is 17 serial round trips to L2 (12 us of
    // fixed cost, measured).  Out-of-range pieces re-read the last one and
    // are not written.
    constexpr int FILL_IT = (N * (LD / 8) + 511) / 512;
    // 16-byte pieces per weight row (a constant in the unrolled kernels)
    const int gpr = NFULL_CT >= 0 ? NFULL_CT * 4 + (TAIL_CT ? 1 : 0) : kpad8 / 8;
    const int total = N * gpr;
    bf16x4 flo[FILL_IT], fhi[FILL_IT];
    for (int j = 0; j < FILL_IT; ++j) {
      const int e = min(tid + j * 512, total - 1);
      const int n = e / gpr;
      const int k = (e - n * gpr) * 8;
      const __bf16* src = Wt + (int64_t)n * K + k;
      const bool hv = k + 8 <= K;  // k + 4 <= K always holds (K % 4 == 0)
      flo[j] = *reinterpret_cast<const bf16x4*>(src);
      fhi[j] = *reinterpret_cast<const bf16x4*>(src + (hv ? 4 : 0));
    }
    for (int j = 0; j < FILL_IT; ++j) {
      const int e = tid + j * 512;
      const int n = e / gpr;
      const int k = (e - n * gpr) * 8;
      if (e < total) {
        const bf16x4 hi = k + 8 <= K ? fhi[j] : bf16x4{};
        *reinterpret_cast<bf16x8*>(&Ws[n * LD + k]) =
            __builtin_shufflevector(flo[j], hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
    }
    if (EPI == 0 && tid < N) bias_s[tid] = bias[tid];
  }
  __syncthreads();

  const __bf16* wrow = &Ws[row_l * LD + kseg * 8];
  f32x4 acc[2][16];
  auto mma_chunk = [&](int k0, const bf16x8& a0, const bf16x8& a1) {
    for (int ni = 0; ni < 16; ++ni) {
      // fence the scheduler every 4 fragments: left alone it hoists the
      // weight reads of all chunks above the MFMAs and spills 2 KB per lane
      if (ni % 4 == 0) __builtin_amdgcn_sched_barrier(0);
      const bf16x8 wf =
          *reinterpret_cast<const bf16x8*>(wrow + ni * 16 * LD + k0);
      acc[0][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a0, acc[0][ni],
                                                           0, 0, 0);
      acc[1][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a1, acc[1][ni],
                                                           0, 0, 0);
    }
  };

  for (int g = blockIdx.x; g * GROUP < M; g += gridDim.x) {
    if (g != (int)blockIdx.x) load_group(g);
    for (int mi = 0; mi < 2; ++mi)
      for (int ni = 0; ni < 16; ++ni) acc[mi][ni] = f32x4{};

    if (NFULL_CT >= 0) {
      for (int kc = 0; kc < NFULL_CT; ++kc) {
        const int slot = kc >= NFULL_CT - LATE ? kc - (NFULL_CT - LATE) : kc;
        mma_chunk(kc * 32, a[slot][0], a[slot][1]);
        if (kc < LATE)  // chunk kc's registers are free again
          for (int mi = 0; mi < 2; ++mi)
            a[kc][mi] = load_full(mi, NFULL_CT - LATE + kc);
        if (TAIL_CT && kc == LATE)
          for (int mi = 0; mi < 2; ++mi) atail[mi] = load_tail(mi);
      }
    } else {
      for (int kc = 0; kc < nfull; ++kc) {
        // unconditional prefetch (the last one re-reads its own chunk): a
        // branch around the loads would cost a full vmcnt(0) per iteration
        const int kn = min(kc + 1, nfull - 1);
        const bf16x8 n0 = load_full(0, kn), n1 = load_full(1, kn);
        mma_chunk(kc * 32, a[0][0], a[0][1]);
        a[0][0] = n0;
        a[0][1] = n1;
      }
    }
    if (ktail) {
      for (int ni = 0; ni < 16; ++ni) {
        bf16x8 wf = *reinterpret_cast<const bf16x8*>(
            &Ws[(ni * 16 + row_l) * LD + w_t_off]);
        if (!w_tv) wf = bf16x8{};
        acc[0][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf, atail[0], acc[0][ni], 0, 0, 0);
        acc[1][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf, atail[1], acc[1][ni], 0, 0, 0);
      }
    }

    // transposed C/D map: lane l, reg r -> row = l&15, col = (l>>4)*4 + r
    for (int mi = 0; mi < 2; ++mi) {
      const int grow = g * GROUP + wave * 32 + mi * 16 + row_l;
      if (grow >= M) continue;
      const int64_t o = (int64_t)grow * N + kseg * 4;
      // all of a row's Yact pieces in flight before the first store: loads
      // and stores share vmcnt, one load per store would serialize them
      bf16x4 y[16];
      if (EPI == 1)
        for (int ni = 0; ni < 16; ++ni)
          y[ni] = *reinterpret_cast<const bf16x4*>(&Yact[o + ni * 16]);
      for (int ni = 0; ni < 16; ++ni) {
        bf16x4 out;
        if (EPI == 0) {
          const f32x4 b =
              *reinterpret_cast<const f32x4*>(&bias_s[ni * 16 + kseg * 4]);
          for (int r = 0; r < 4; ++r)
            out[r] = f2bf(epi_bias_tanh(acc[mi][ni][r], b[r]));
        } else {
          for (int r = 0; r < 4; ++r)
            out[r] = f2bf(epi_dtanh(acc[mi][ni][r], y[ni][r]));
        }
        *reinterpret_cast<bf16x4*>(&C[o + ni * 16]) = out;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad partials: dW[K,N] = X^T @ dY, split over M into SLABS partial sums.
// Each block: one (ktile, ntile, slab); loops its M-chunk with MFMA where
// logical A = X^T [K, M] (i.e. A[k][m] = X[m][k]), logical B = dY [M, N].
// Deterministic: fixed slab count + ordered tree reduce (no atomics).
// Partials: f32 [S, K, N]; db partials f32 [S, N] (bias grad = colsum dY).
// Tiles are staged in NATURAL [m][k] / [m][n] layout with fully-coalesced
// bf16x8 global loads; the transpose happens at the MFMA fragment reads from
// LDS (scalar LDS reads are cheap; strided 2-byte GLOBAL reads were the
// bottleneck of the first version of this kernel).
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// glds wgrad, 64x64 output tile, BKm=64 m-chunks: stages both operand
// chunks with __builtin_amdgcn_global_load_lds (16B per lane, LDS image
// linear in lane order — guide §5: 64²-tile step-3 structure), two LDS
// buffers, one __syncthreads per chunk (the barrier's vmcnt(0) drains the
// in-flight glds of the NEXT chunk — the simple 2-barrier recipe).
// Requires full, aligned tiles: bk+64<=K, bn+64<=N and a full 64-row
// m-chunk; the launcher falls back to the register-staged kernel for edge
// tiles (K%64 tails, the head layer's N=4, partial slabs).
// ---------------------------------------------------------------------------
template <bool WANT_DB, int FK, int FN, bool A_PERM = false>
__global__ __launch_bounds__(256) void wgrad_glds_kernel(
    const __bf16* __restrict__ X, const __bf16* __restrict__ dY,
    float* __restrict__ dW_part, float* __restrict__ db_part,
    int M, int N, int K, int slabs, FeistelMap fm = FeistelMap{}) {
  constexpr int BKm = 64;
  constexpr int TK = 32 * FK, TN = 32 * FN;
  // UNPADDED linear images (glds cannot scatter past a row pad)
  __shared__ __bf16 Xs[2][BKm][TK];
  __shared__ __bf16 Ys[2][BKm][TN];

  const int bk = blockIdx.x * TK;
  const int bn = blockIdx.y * TN;
  const int slab = blockIdx.z;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;

  const int m_per_slab = (M + slabs - 1) / slabs;
  const int m_begin = slab * m_per_slab;
  const int m_end = min(M, m_begin + m_per_slab);
  const int nchunks = (m_end - m_begin) / BKm;  // full chunks only (caller
                                                // guarantees divisibility)
  f32x4 acc[FK][FN] = {};
  float db_acc = 0.f;

  // gather+wgrad fusion: X rows go through the epoch permutation
  uint64_t fkey = 0;
  uint32_t fmb = 0;
  if (A_PERM) fkey = feistel_key(fm, &fmb);
  auto x_row = [&](int gm) -> int64_t {
    return A_PERM ? feistel_src_row(fm, fkey, fmb, gm) : (int64_t)gm;
  };

  // partial-K final tile (e.g. obs_dim=260 with TK=160: second tile covers
  // 100 live columns): X staged with guarded register loads instead of
  // glds — the K TAIL no longer needs a second full pass over dY
  // (profiles/lstm_kernel_stats_r2b.txt: the tail kernel re-read all of
  // dgates for 4 columns, ~1.5 ms/update).
  const bool k_tail = bk + TK > K;

  // one glds instruction stages 64 lanes x 16B = 1KB = 512 bf16; a 64xTW
  // chunk is 64*TW*2 B = TW/8 instructions = TW/32 per wave.
  auto glds_chunk = [&](int buf, int m0) {
    for (int j = 0; j < FK; ++j) {
      const int e0 = (wave * FK + j) * 512;
      const int row = (e0 + lane * 8) / TK;
      const int col = (e0 + lane * 8) % TK;
      if (k_tail) {
        bf16x8 v = bf16x8{};
        const int gk = bk + col;
        const int64_t xr = x_row(m0 + row) * K;
        if (gk + 8 <= K) {
          v = *reinterpret_cast<const bf16x8*>(&X[xr + gk]);
        } else {
          for (int i = 0; i < 8; ++i)
            v[i] = (gk + i < K) ? X[xr + gk + i] : (__bf16)0.f;
        }
        *reinterpret_cast<bf16x8*>(&Xs[buf][0][0] + e0 + lane * 8) = v;
        continue;
      }
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &X[x_row(m0 + row) * K + bk + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &Xs[buf][0][0] + e0),
          16, 0, 0);
    }
    for (int j = 0; j < FN; ++j) {
      const int e0 = (wave * FN + j) * 512;
      const int row = (e0 + lane * 8) / TN;
      const int col = (e0 + lane * 8) % TN;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &dY[(int64_t)(m0 + row) * N + bn + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &Ys[buf][0][0] + e0),
          16, 0, 0);
    }
  };

  const int row_a = lane & 15;
  const int kseg = lane >> 4;

  if (nchunks > 0) glds_chunk(0, m_begin);
  __syncthreads();  // vmcnt(0) inside the barrier drains the glds
  for (int ci = 0; ci < nchunks; ++ci) {
    const int cur = ci & 1;
    if (ci + 1 < nchunks) glds_chunk(1 - cur, m_begin + (ci + 1) * BKm);

    if (WANT_DB && tid < TN) {
      float s = 0.f;
      for (int i = 0; i < BKm; ++i) s += bf2f(Ys[cur][i][tid]);
      db_acc += s;
    }
    // two 32-row reduction batches per 64-row chunk
    for (int half = 0; half < 2; ++half) {
      const int mb = half * 32;
      bf16x8 af[FK], bf_[FN];
      for (int fi = 0; fi < FK; ++fi)
        for (int i = 0; i < 8; ++i)
          af[fi][i] =
              Xs[cur][mb + kseg * 8 + i][wr * (16 * FK) + fi * 16 + row_a];
      for (int ni = 0; ni < FN; ++ni)
        for (int i = 0; i < 8; ++i)
          bf_[ni][i] =
              Ys[cur][mb + kseg * 8 + i][wc * (16 * FN) + ni * 16 + row_a];
      for (int fi = 0; fi < FK; ++fi)
        for (int ni = 0; ni < FN; ++ni)
          acc[fi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[fi], bf_[ni], acc[fi][ni], 0, 0, 0);
    }
    __syncthreads();
  }

  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  float* out = dW_part + (int64_t)slab * K * N;
  for (int fi = 0; fi < FK; ++fi)
    for (int ni = 0; ni < FN; ++ni) {
      const int gcol = bn + wc * (16 * FN) + ni * 16 + ccol;
      for (int r = 0; r < 4; ++r) {
        const int grow = bk + wr * (16 * FK) + fi * 16 + crow_base + r;
        if (grow < K) out[(int64_t)grow * N + gcol] = acc[fi][ni][r];
      }
    }
  if (WANT_DB && tid < TN && blockIdx.x == 0)
    db_part[(int64_t)slab * N + bn + tid] = db_acc;
}

template <bool WANT_DB, int FK, int FN, bool A_PERM = false>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(
    const __bf16* __restrict__ X, const __bf16* __restrict__ dY,
    float* __restrict__ dW_part, float* __restrict__ db_part,
    int M, int N, int K, int slabs, int kt0, FeistelMap fm = FeistelMap{}) {
  // FK/FN = MFMA fragments per wave along K/N: block tile (32*FK) x (32*FN)
  // over the dW output; reduction dim is M, chunked BKm=32 rows at a time
  // with double-buffered natural-layout LDS staging (coalesced bf16x8
  // global loads; the transpose happens at the fragment reads).
  constexpr int BKm = 32;
  constexpr int TK = 32 * FK, TN = 32 * FN;
  constexpr int LDX = TK + 8, LDY = TN + 8;
  __shared__ __bf16 Xs[2][BKm][LDX];   // X tile, natural layout: [m][k]
  __shared__ __bf16 Ys[2][BKm][LDY];   // dY tile, natural layout: [m][n]

  const int bk = (kt0 + blockIdx.x) * TK;
  const int bn = blockIdx.y * TN;
  const int slab = blockIdx.z;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;

  const int m_per_slab = (M + slabs - 1) / slabs;
  const int m_begin = slab * m_per_slab;
  const int m_end = min(M, m_begin + m_per_slab);

  f32x4 acc[FK][FN] = {};
  float db_acc = 0.f;

  uint64_t fkey = 0;
  uint32_t fmb = 0;
  if (A_PERM) fkey = feistel_key(fm, &fmb);

  bf16x8 rx[FK / 2], ry[FN / 2];
  auto load_chunk = [&](int m0) {
    // X chunk [32 m][TK k]: 32*TK elems = 256 threads * (FK/2) vec8
    for (int j = 0; j < FK / 2; ++j) {
      const int c = tid + j * 256;          // chunk id over [32][TK/8]
      const int m = c / (4 * FK);
      const int c8 = (c % (4 * FK)) * 8;
      rx[j] = bf16x8{};
      const int gm = m0 + m;
      if (gm < m_end) {
        const int64_t sm = A_PERM ? feistel_src_row(fm, fkey, fmb, gm)
                                  : (int64_t)gm;
        const int gk = bk + c8;
        if (gk + 8 <= K) {
          rx[j] = *reinterpret_cast<const bf16x8*>(&X[sm * K + gk]);
        } else {
          for (int i = 0; i < 8; ++i)
            rx[j][i] = (gk + i < K) ? X[sm * K + gk + i] : (__bf16)0.f;
        }
      }
    }
    for (int j = 0; j < FN / 2; ++j) {
      const int c = tid + j * 256;
      const int m = c / (4 * FN);
      const int c8 = (c % (4 * FN)) * 8;
      ry[j] = bf16x8{};
      const int gm = m0 + m;
      if (gm < m_end) {
        const int gn = bn + c8;
        if (gn + 8 <= N) {
          ry[j] = *reinterpret_cast<const bf16x8*>(&dY[(int64_t)gm * N + gn]);
        } else {
          for (int i = 0; i < 8; ++i)
            ry[j][i] = (gn + i < N) ? dY[(int64_t)gm * N + gn + i] : (__bf16)0.f;
        }
      }
    }
  };
  auto store_chunk = [&](int buf) {
    for (int j = 0; j < FK / 2; ++j) {
      const int c = tid + j * 256;
      *reinterpret_cast<bf16x8*>(&Xs[buf][c / (4 * FK)][(c % (4 * FK)) * 8]) = rx[j];
    }
    for (int j = 0; j < FN / 2; ++j) {
      const int c = tid + j * 256;
      *reinterpret_cast<bf16x8*>(&Ys[buf][c / (4 * FN)][(c % (4 * FN)) * 8]) = ry[j];
    }
  };

  const int row_a = lane & 15;
  const int kseg = lane >> 4;
  const int nchunks = (m_end - m_begin + BKm - 1) / BKm;

  if (nchunks > 0) {
    load_chunk(m_begin);
    store_chunk(0);
    __syncthreads();
  }
  for (int ci = 0; ci < nchunks; ++ci) {
    const int cur = ci & 1;
    const int m0 = m_begin + ci * BKm;
    if (ci + 1 < nchunks) load_chunk(m0 + BKm);

    if (WANT_DB && tid < TN) {
      float s = 0.f;
      for (int i = 0; i < BKm && m0 + i < m_end; ++i)
        s += bf2f(Ys[cur][i][tid]);
      db_acc += s;
    }
    // fragment reads do the transpose: logical A[kout][m] = X[m][kout],
    // logical B[m][n] = dY[m][n]; reduction index m = kseg*8 + i.
    bf16x8 af[FK], bf_[FN];
    for (int fi = 0; fi < FK; ++fi)
      for (int i = 0; i < 8; ++i)
        af[fi][i] = Xs[cur][kseg * 8 + i][wr * (16 * FK) + fi * 16 + row_a];
    for (int ni = 0; ni < FN; ++ni)
      for (int i = 0; i < 8; ++i)
        bf_[ni][i] = Ys[cur][kseg * 8 + i][wc * (16 * FN) + ni * 16 + row_a];
    for (int fi = 0; fi < FK; ++fi)
      for (int ni = 0; ni < FN; ++ni)
        acc[fi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[fi], bf_[ni], acc[fi][ni], 0, 0, 0);

    if (ci + 1 < nchunks) store_chunk(1 - cur);
    __syncthreads();
  }

  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  float* out = dW_part + (int64_t)slab * K * N;
  for (int fi = 0; fi < FK; ++fi)
    for (int ni = 0; ni < FN; ++ni) {
      const int gcol = bn + wc * (16 * FN) + ni * 16 + ccol;
      if (gcol >= N) continue;
      for (int r = 0; r < 4; ++r) {
        const int grow = bk + wr * (16 * FK) + fi * 16 + crow_base + r;
        if (grow >= K) continue;
        out[(int64_t)grow * N + gcol] = acc[fi][ni][r];
      }
    }
  if (WANT_DB && tid < TN && kt0 == 0 && blockIdx.x == 0) {
    const int gn = bn + tid;
    if (gn < N) db_part[(int64_t)slab * N + gn] = db_acc;
  }
}

__global__ void slab_reduce_kernel(const float* __restrict__ part,
                                   float* __restrict__ out, int64_t elems,
                                   int slabs) {
  // float4 per thread + 4-way unrolled slab loop (keeps >=16 loads in
  // flight; the scalar version was latency-bound on the slab chain).
  const int64_t nvec = elems >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 s0 = {}, s1 = {}, s2 = {}, s3 = {};
    int k = 0;
    for (; k + 4 <= slabs; k += 4) {
      s0 += *reinterpret_cast<const f32x4*>(&part[(int64_t)k * elems + i * 4]);
      s1 += *reinterpret_cast<const f32x4*>(&part[(int64_t)(k + 1) * elems + i * 4]);
      s2 += *reinterpret_cast<const f32x4*>(&part[(int64_t)(k + 2) * elems + i * 4]);
      s3 += *reinterpret_cast<const f32x4*>(&part[(int64_t)(k + 3) * elems + i * 4]);
    }
    for (; k < slabs; ++k)
      s0 += *reinterpret_cast<const f32x4*>(&part[(int64_t)k * elems + i * 4]);
    // fixed association order: (s0 + s1) + (s2 + s3) — deterministic
    *reinterpret_cast<f32x4*>(&out[i * 4]) = (s0 + s1) + (s2 + s3);
  }
  // scalar tail
  for (int64_t i = (nvec << 2) + blockIdx.x * blockDim.x + threadIdx.x;
       i < elems; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < slabs; ++k) s += part[(int64_t)k * elems + i];
    out[i] = s;
  }
}

// tiny-elems variant (e.g. the head bias, elems=4, slabs up to 256): one
// block per element, threads parallel over slabs, deterministic tree reduce.
__global__ void slab_reduce_small_kernel(const float* __restrict__ part,
                                         float* __restrict__ out,
                                         int64_t elems, int slabs) {
  __shared__ float red[256];
  const int64_t e = blockIdx.x;
  if (e >= elems) return;
  float s = 0.f;
  for (int k = threadIdx.x; k < slabs; k += 256)
    s += part[(int64_t)k * elems + e];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[e] = red[0];
}

// ---------------------------------------------------------------------------
// bf16 transpose: dst[N,K] = src[K,N]^T.  Keeps per-weight transposed
// mirrors fresh after each Adam step so every model GEMM can stage its B
// operand with contiguous vector loads (TRANS_B path) — the strided
// alternative spilled registers and ran 6x slower.  LDS 64x64 tile.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_bf16_kernel(
    const __bf16* __restrict__ src, __bf16* __restrict__ dst, int K, int N) {
  __shared__ __bf16 tile[64][64 + 4];
  const int kb = blockIdx.x * 64;
  const int nb = blockIdx.y * 64;
  // load 64x64 tile of src (rows k, cols n), coalesced along n
  for (int e = threadIdx.x; e < 64 * 8; e += 256) {
    const int r = e >> 3;            // 0..63 (k)
    const int c8 = (e & 7) * 8;      // 0..56 (n)
    const int gk = kb + r;
    const int gn = nb + c8;
    bf16x8 v = {};
    if (gk < K) {
      if (gn + 8 <= N) {
        v = *reinterpret_cast<const bf16x8*>(&src[(int64_t)gk * N + gn]);
      } else {
        for (int i = 0; i < 8; ++i)
          v[i] = (gn + i < N) ? src[(int64_t)gk * N + gn + i] : (__bf16)0.f;
      }
    }
    *reinterpret_cast<bf16x8*>(&tile[r][c8]) = v;
  }
  __syncthreads();
  // write transposed, coalesced along k
  for (int e = threadIdx.x; e < 64 * 8; e += 256) {
    const int r = e >> 3;            // 0..63 (n)
    const int c8 = (e & 7) * 8;      // 0..56 (k)
    const int gn = nb + r;
    const int gk = kb + c8;
    if (gn >= N) continue;
    if (gk + 8 <= K) {
      bf16x8 v;
      for (int i = 0; i < 8; ++i) v[i] = tile[c8 + i][r];
      *reinterpret_cast<bf16x8*>(&dst[(int64_t)gn * K + gk]) = v;
    } else {
      for (int i = 0; i < 8 && gk + i < K; ++i)
        dst[(int64_t)gn * K + gk + i] = tile[c8 + i][r];
    }
  }
}

// ---------------------------------------------------------------------------
// elementwise casts
// ---------------------------------------------------------------------------
__global__ void f32_to_bf16_kernel(const float* __restrict__ in,
                                   __bf16* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = f2bf(in[i]);
}

// ---------------------------------------------------------------------------
// GAE backward scan (per env): adv[t] = delta_t + gamma*lam*(1-done_t)*adv[t+1]
// rewards/values/dones laid out [T, N] so lane reads coalesce across envs.
// ---------------------------------------------------------------------------
__global__ void gae_kernel(const float* __restrict__ rewards,
                           const float* __restrict__ values,   // [T+1, N]
                           const bool* __restrict__ dones,     // [T, N]
                           float* __restrict__ adv, float* __restrict__ ret,
                           int T, int N, float gamma, float lam) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float running = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const float nonterm = dones[(int64_t)t * N + n] ? 0.f : 1.f;
    const float delta = rewards[(int64_t)t * N + n] +
                        gamma * values[(int64_t)(t + 1) * N + n] * nonterm -
                        values[(int64_t)t * N + n];
    running = delta + gamma * lam * nonterm * running;
    adv[(int64_t)t * N + n] = running;
    ret[(int64_t)t * N + n] = running + values[(int64_t)t * N + n];
  }
}

// ---------------------------------------------------------------------------
// Fused Adam (f32 master params; bf16 mirror refreshed in the same pass)
// ---------------------------------------------------------------------------
// clip_part/nparts/max_norm: when given, every block tree-reduces the
// sumsq partials itself and derives the clip scale inline (the partials
// are ~1 KB, L2-resident) — this removed the separate one-block
// clip_scale launch from the 32x-per-update optimizer chain.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            __bf16* __restrict__ p_bf16, int64_t n, float lr,
                            float beta1, float beta2, float eps, float bc1,
                            float bc2, const float* __restrict__ gscale,
                            const int* __restrict__ step_ctr,
                            const float* __restrict__ clip_part, int nparts,
                            float max_norm) {
  if (step_ctr) {
    // device step counter (hipGraph-replayable): effective step = *ctr + 1;
    // the companion increment kernel advances it after this launch.
    const float st = (float)(*step_ctr + 1);
    bc1 = 1.f - powf(beta1, st);
    bc2 = 1.f - powf(beta2, st);
  }
  float s = 1.f;
  if (clip_part) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += clip_part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    const float norm = sqrtf(red[0]);
    s = (max_norm > 0.f && norm > max_norm) ? max_norm / norm : 1.f;
  } else if (gscale) {
    s = *gscale;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * s;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / bc1;
    const float vhat = vi / bc2;
    const float pi = p[i] - lr * mhat / (sqrtf(vhat) + eps);
    p[i] = pi;
    if (p_bf16) p_bf16[i] = f2bf(pi);
  }
}

// grad-norm^2: deterministic two-pass (fixed grid of partials, ordered sum)
__global__ void sumsq_partial_kernel(const float* __restrict__ g, int64_t n,
                                     float* __restrict__ part) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    s += g[i] * g[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void clip_scale_kernel(const float* __restrict__ part, int nparts,
                                  float max_norm, float* __restrict__ scale) {
  // one block of 256; tree reduce (deterministic, ~4x faster than the
  // single-thread serial loop this replaced)
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = sqrtf(red[0]);
    *scale = (max_norm > 0.f && norm > max_norm) ? max_norm / norm : 1.f;
  }
}

// ---------------------------------------------------------------------------
// Fused optimizer tail.
//
// Last-block ticket: folds a "+delta" counter advance into the kernel that
// reads the counter.  Every thread of every block has loaded the counter
// (the value is in its register) and passed a workgroup barrier before
// thread 0 draws its ticket, so the block that draws gridDim-1 knows every
// reader is done; it stores the new value and rearms the ticket (graph
// replays start from 0 again).  The draw is a relaxed agent-scope atomic
// with NO __threadfence(): nothing this launch wrote has to be visible to
// the other blocks, only the order "all loads returned -> store" matters,
// and the fence (an L2 write-back plus an L1 invalidate per block) measured
// 15.4 us for the 522-block Adam launch against 5.5 us without a ticket.
// Draw early, commit late: the atomic's round trip overlaps the block's
// own work.
// ---------------------------------------------------------------------------
GFX_DEV unsigned int ticket_draw(unsigned int* ticket) {
  return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
GFX_DEV void ticket_commit(unsigned int drawn, T* ctr, T old, T delta,
                           unsigned int* ticket) {
  if (drawn == gridDim.x - 1u) {
    *ctr = old + delta;
    *ticket = 0u;
  }
}

// grads_finalize_kernel: every wgrad slab workspace of one backward pass
// reduced into the flat gradient buffer in ONE launch, bit-for-bit in the
// association order of slab_reduce_kernel / slab_reduce_small_kernel, plus
// (optionally) the 256 sum-of-squares partials sumsq_partial_kernel would
// write for the same buffer.
//
// Layout: 256 blocks x 1024 threads.  Thread (q = tid>>8, t = tid&255) of
// block b works on elements i = b*256 + t + j*65536 — exactly the elements
// sumsq_partial_kernel's block b / thread t squares, in the same j order —
// and the four q-threads of an element split its slab sum:
//   vector path (elems > 4096, e < elems&~3): q sums slabs k = q, q+4, ...
//     (the s0..s3 interleave), q = 0 adds the slabs%4 remainder, combined
//     as (s0+s1)+(s2+s3);
//   scalar tail (e >= elems&~3): q = 0 sums serially over k;
//   small path: the 256 leaves of the halving tree are the serial sums over
//     k = t', t'+256, ...; q reduces leaves t' = q+4m through tree widths
//     128..4 in registers (m-space widths 32..1), the widths 2 and 1 are
//     (v0+v2)+(v1+v3).
// Each thread streams its slab column with up to 32 independent loads in
// flight (the kernel is latency-bound below that: 16 waves per CU, one
// block per CU).
__global__ __launch_bounds__(1024) void grads_finalize_kernel(
    FinalizeTable tab, float* __restrict__ grads, int64_t n,
    float* __restrict__ clip_part) {
  __shared__ float comb[4][256];
  const int t = threadIdx.x & 255;
  const int q = threadIdx.x >> 8;
  float sq = 0.f;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n;
       base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + t;
    const float* part = nullptr;
    int64_t elems = 0, e = 0;
    int slabs = 0, small = 0;
#pragma unroll
    for (int s = 0; s < kMaxFinalizeSegs; ++s) {
      const int64_t d = i - tab.seg[s].off;
      if (s < tab.nseg && i < n && d >= 0 && d < tab.seg[s].elems) {
        part = tab.seg[s].part;
        elems = tab.seg[s].elems;
        e = d;
        slabs = tab.seg[s].slabs;
        small = tab.seg[s].small;
      }
    }
    int kind = -1;  // 0 vector path, 1 scalar tail, 2 small tree
    float val = 0.f;
    if (part) {
      const float* pe = part + e;
      if (small) {
        kind = 2;
        // leaf m = serial sum over k = q+4m, +256, ...; a slab past the
        // end adds +0.f, which leaves the sum's bits alone (its load is
        // clamped in bounds and discarded).  16 loads in flight per round.
        float r[64];
#pragma unroll
        for (int m = 0; m < 64; ++m) r[m] = 0.f;
#pragma unroll
        for (int h = 0; h < 64; h += 16) {
          for (int k0 = q + 4 * h; k0 < slabs; k0 += 256) {
            float x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
              x[u] = pe[(int64_t)min(k0 + 4 * u, slabs - 1) * elems];
#pragma unroll
            for (int u = 0; u < 16; ++u)
              r[h + u] += (k0 + 4 * u < slabs) ? x[u] : 0.f;
          }
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1)
#pragma unroll
          for (int m = 0; m < w; ++m) r[m] += r[m + w];
        val = r[0];
      } else if (e < (elems & ~(int64_t)3)) {
        kind = 0;
        const int kend = slabs & ~3;
        float s = 0.f;
        int k = q;
        for (; k + 124 < kend; k += 128) {
          float x[32];
#pragma unroll
          for (int u = 0; u < 32; ++u) x[u] = pe[(int64_t)(k + 4 * u) * elems];
#pragma unroll
          for (int u = 0; u < 32; ++u) s += x[u];
        }
        for (; k + 60 < kend; k += 64) {
          float x[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) x[u] = pe[(int64_t)(k + 4 * u) * elems];
#pragma unroll
          for (int u = 0; u < 16; ++u) s += x[u];
        }
        for (; k < kend; k += 4) s += pe[(int64_t)k * elems];
        if (q == 0)
          for (k = kend; k < slabs; ++k) s += pe[(int64_t)k * elems];
        val = s;
      } else {
        kind = 1;
        if (q == 0) {
          float s = 0.f;
          for (int k = 0; k < slabs; ++k) s += pe[(int64_t)k * elems];
          val = s;
        }
      }
    }
    comb[q][t] = val;
    __syncthreads();
    if (q == 0 && i < n) {
      float g;
      if (kind == 0)
        g = (comb[0][t] + comb[1][t]) + (comb[2][t] + comb[3][t]);
      else if (kind == 2)
        g = (comb[0][t] + comb[2][t]) + (comb[1][t] + comb[3][t]);
      else if (kind == 1)
        g = val;
      else
        g = grads[i];  // not covered by any segment: left as it is
      if (kind >= 0) grads[i] = g;
      sq += g * g;
    }
    __syncthreads();
  }
  if (clip_part) {
    // block b's partial: same per-thread serial sums, same halving tree
    __shared__ float red[256];
    if (q == 0) red[t] = sq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (q == 0 && t < w) red[t] += red[t + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) clip_part[blockIdx.x] = red[0];
  }
}

// adam_tail_kernel: adam_kernel with the two launches that followed it
// folded in.  (1) For an element inside a [K,N] weight segment the bf16
// value written to p_bf16[i] is stored a second time at mirror[n*K + k],
// which is what transpose_bf16_kernel produced from p_bf16 (the whole model
// is a few hundred KB, so the scattered 2-byte stores stay in L2).  (2) The
// step counter is advanced by the last-block ticket instead of the
// increment kernel.  The per-element update is adam_kernel's, expression
// for expression.
__global__ __launch_bounds__(1024) void adam_tail_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, __bf16* __restrict__ p_bf16, int64_t n, float lr,
    float beta1, float beta2, float eps, int* step_ctr,
    unsigned int* ticket, const float* __restrict__ clip_part, int nparts,
    float max_norm, MirrorTable mt) {
  // 1024-thread blocks (adam_kernel: 256): a quarter of the tickets to
  // draw; the per-element update does not depend on the launch geometry.
  const int ctr = *(volatile const int*)step_ctr;
  __syncthreads();
  unsigned int drawn = 0;
  const bool drawer = ticket && threadIdx.x == 0;
  if (drawer) drawn = ticket_draw(ticket);
  const float st = (float)(ctr + 1);
  const float bc1 = 1.f - powf(beta1, st);
  const float bc2 = 1.f - powf(beta2, st);
  float s = 1.f;
  if (clip_part) {
    // adam_kernel's 256-thread tree, run by the first 256 threads
    __shared__ float red[256];
    if (threadIdx.x < 256) {
      float acc = 0.f;
      for (int i = threadIdx.x; i < nparts; i += 256) acc += clip_part[i];
      red[threadIdx.x] = acc;
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    const float norm = sqrtf(red[0]);
    s = (max_norm > 0.f && norm > max_norm) ? max_norm / norm : 1.f;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * s;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / bc1;
    const float vhat = vi / bc2;
    const float pi = p[i] - lr * mhat / (sqrtf(vhat) + eps);
    p[i] = pi;
    const __bf16 pb = f2bf(pi);
    if (p_bf16) p_bf16[i] = pb;
#pragma unroll
    for (int sgi = 0; sgi < kMaxMirrorSegs; ++sgi) {
      const int64_t d = i - mt.seg[sgi].off;
      if (sgi < mt.nseg && d >= 0 &&
          d < (int64_t)mt.seg[sgi].K * mt.seg[sgi].N) {
        const unsigned K = (unsigned)mt.seg[sgi].K, N = (unsigned)mt.seg[sgi].N;
        const unsigned k = (unsigned)d / N;
        const unsigned c = (unsigned)d - k * N;
        reinterpret_cast<__bf16*>(mt.seg[sgi].dst)[(int64_t)c * K + k] = pb;
      }
    }
  }
  if (drawer) ticket_commit(drawn, step_ctr, ctr, 1, ticket);
}

// ---------------------------------------------------------------------------
// Categorical sampling + logp + entropy from the fused head output
// head[M, A+1] f32: cols 0..A-1 logits, col A value.
// Counter-based RNG (splitmix64): deterministic in (seed, step, env).
// ---------------------------------------------------------------------------
__global__ void sample_head_kernel(const float* __restrict__ head, int M,
                                   int n_actions, uint64_t seed, uint64_t step,
                                   int64_t* __restrict__ actions,
                                   float* __restrict__ logp,
                                   float* __restrict__ value,
                                   float* __restrict__ entropy,
                                   int greedy,
                                   const unsigned long long* __restrict__ step_base,
                                   int row_offset) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  if (step_base) step += *step_base;  // device counter: hipGraph-replayable RNG
  const int64_t mg = m + row_offset;  // global row: split launches keep RNG
  const float* row = head + (int64_t)m * (n_actions + 1);
  const float logz = head_logz(row, n_actions);

  int a = 0;
  if (greedy) {
    float best = row[0];
    for (int j = 1; j < n_actions; ++j)
      if (row[j] > best) { best = row[j]; a = j; }
  } else {
    a = sample_categorical(row, n_actions, logz, seed, step, mg);
  }
  actions[m] = a;
  logp[m] = row[a] - logz;
  if (value) value[m] = row[n_actions];
  if (entropy) {
    float h = 0.f;
    for (int j = 0; j < n_actions; ++j) {
      const float lp = row[j] - logz;
      h -= fast_exp(lp) * lp;
    }
    entropy[m] = h;
  }
}

// ---------------------------------------------------------------------------
// PPO clipped-surrogate loss backward: head[M, A+1] f32 -> dhead[M, A+1] bf16
// losses (logging): [pi_loss, v_loss, entropy, approx_kl, clipfrac] via
// block-partial + atomicAdd (logging only; gradients are deterministic).
// ---------------------------------------------------------------------------
// One row of the loss backward, shared by ppo_loss_bwd_kernel and
// head_loss_bwd_kernel so both produce the same bits: row = the row's
// n_actions logits and its value, drow = where its gradient goes.
GFX_DEV void ppo_loss_row(const float* row, __bf16* drow, int a, float olp,
                          float A, float rt, int n_actions, float clip_eps,
                          float ent_coef, float vf_coef, float inv_count,
                          float& l_pi, float& l_v, float& l_ent, float& l_kl,
                          float& l_clip) {
  float mx = row[0];
  for (int j = 1; j < n_actions; ++j) mx = fmaxf(mx, row[j]);
  float z = 0.f;
  for (int j = 0; j < n_actions; ++j) z += expf(row[j] - mx);
  const float logz = logf(z) + mx;
  const float lp = row[a] - logz;
  const float ratio = expf(lp - olp);
  const bool clipped = (ratio > 1.f + clip_eps) || (ratio < 1.f - clip_eps);
  const float surr1 = ratio * A;
  const float rclip = fminf(fmaxf(ratio, 1.f - clip_eps), 1.f + clip_eps);
  const float surr2 = rclip * A;
  // d(-min(surr1,surr2))/dlogp = -A*ratio when surr1 <= surr2 (unclipped
  // branch active), else 0
  const float g_lp = (surr1 <= surr2) ? (-A * ratio) : 0.f;
  // entropy bonus: loss += -ent_coef * H
  float H = 0.f;
  for (int j = 0; j < n_actions; ++j) {
    const float lpj = row[j] - logz;
    H -= expf(lpj) * lpj;
  }
  for (int j = 0; j < n_actions; ++j) {
    const float pj = expf(row[j] - logz);
    const float onehot = (j == a) ? 1.f : 0.f;
    float d = g_lp * (onehot - pj);             // policy term
    d += ent_coef * pj * ((row[j] - logz) + H);  // -ent_coef*dH/dlogit
    drow[j] = f2bf(d * inv_count);
  }
  const float v = row[n_actions];
  const float dv = vf_coef * (v - rt);
  drow[n_actions] = f2bf(dv * inv_count);

  l_pi = -fminf(surr1, surr2);
  l_v = 0.5f * (v - rt) * (v - rt);
  l_ent = H;
  l_kl = olp - lp;
  l_clip = clipped ? 1.f : 0.f;
}

__global__ void ppo_loss_bwd_kernel(
    const float* __restrict__ head, const int64_t* __restrict__ actions,
    const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ ret, __bf16* __restrict__ dhead, int M,
    int n_actions, float clip_eps, float ent_coef, float vf_coef,
    float inv_count, float* __restrict__ losses) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float l_pi = 0.f, l_v = 0.f, l_ent = 0.f, l_kl = 0.f, l_clip = 0.f;
  if (m < M)
    ppo_loss_row(head + (int64_t)m * (n_actions + 1),
                 dhead + (int64_t)m * (n_actions + 1), (int)actions[m],
                 old_logp[m], adv[m], ret[m], n_actions, clip_eps, ent_coef,
                 vf_coef, inv_count, l_pi, l_v, l_ent, l_kl, l_clip);
  // block reduction for logging scalars
  __shared__ float red[256];
  float vals[5] = {l_pi, l_v, l_ent, l_kl, l_clip};
  for (int s = 0; s < 5; ++s) {
    red[threadIdx.x] = vals[s];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0 && losses) atomicAdd(&losses[s], red[0] * inv_count);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// head_loss_bwd_kernel: the head layer of the MLP update in ONE pass over
// h2 — head GEMM (h2 @ W3 + b3), PPO loss backward, W3/b3 wgrad slab
// partials and the head dgrad (dh2 = dhead @ W3^T * (1 - h2^2)).  It stands
// for the launch sequence
//   gemm_kernel<true,0,false,true,2>      head  = h2 @ W3t^T + b3
//   ppo_loss_bwd_kernel                   dhead = dL/dhead
//   wgrad_partial_kernel<true,2,2>        W3/b3 slab partials
//   gemm_kernel<true,1,true,false,2>      dh2
// and every output is BITWISE what that sequence writes: each MFMA output
// element sees the same (a,b) products at the same k positions on top of
// the same accumulator, in the same order —
//   head : 8 sequential 16x16x32 steps over k = 0..255, bias added after;
//   dW3  : one step per 32-row chunk counted from the slab's first row,
//          reduction index kseg*8+i inside the chunk, rows past the slab
//          end zero;
//   dh2  : one step, dhead at k = 0..head_dim-1 and zeros above;
// the per-row loss math is ppo_loss_row for both kernels.
//
// One block owns one wgrad slab (rows [slab*mps, min(M, (slab+1)*mps)),
// mps = ceil(M/slabs) <= 128) and keeps its h2 rows in LDS: staged once
// (glds 16 B when the slab is a full 128 rows), read by the head MFMAs, by
// the transposing wgrad fragment reads and by the tanh' epilogue, which
// writes dh2 over the h2 element it just read; the tile then leaves with
// 16 B stores.  The tile is XOR-swizzled in 16 B chunks (chunk c of row r
// sits at c ^ (r & 15)): rows are 512 B apart, so unswizzled every row of
// a fragment read would start in the same bank.  glds writes LDS linearly
// in lane order, so the swizzle is applied to the per-lane SOURCE address.
// LDS: 64 KB tile + head f32 [128][17] + dhead bf16 [128][16] = 76.5 KB,
// two blocks per CU.
// ---------------------------------------------------------------------------
constexpr int kHlbRows = 128;   // rows per block (max m_per_slab)
constexpr int kHlbHid = 256;    // hidden width (tile row length)
constexpr int kHlbHead = 16;    // max head_dim (one MFMA n/k fragment)
constexpr int kHlbHdLd = kHlbHead + 1;  // head f32 row stride (bank spread)
constexpr int kLossShardLd = 32;  // floats per logging-sum shard: one 128 B line

// element offset of (row r, column col) in the swizzled h2 tile
GFX_DEV int hlb_off(int r, int col) {
  const int c = col >> 3;
  return r * kHlbHid + (((c & 16) | ((c ^ r) & 15)) << 3) + (col & 7);
}

__global__ __launch_bounds__(256, 2) void head_loss_bwd_kernel(
    const __bf16* __restrict__ h2, const __bf16* __restrict__ W3t,
    const __bf16* __restrict__ W3, const float* __restrict__ b3,
    const int64_t* __restrict__ actions, const float* __restrict__ old_logp,
    const float* __restrict__ adv, const float* __restrict__ ret,
    float* __restrict__ head, __bf16* __restrict__ dhead,
    __bf16* __restrict__ dh2, float* __restrict__ dW_part,
    float* __restrict__ db_part, int M, int head_dim, int slabs,
    float clip_eps, float ent_coef, float vf_coef, float inv_count,
    float* __restrict__ losses, int loss_shards) {
  // ONE shared object (a second one beside a glds target can make the
  // compiler drain vmcnt before every LDS read)
  constexpr int kTileBytes = kHlbRows * kHlbHid * 2;
  constexpr int kHdBytes = kHlbRows * kHlbHdLd * 4;
  constexpr int kDsBytes = kHlbRows * kHlbHead * 2;
  __shared__ __align__(16) unsigned char smem[kTileBytes + kHdBytes + kDsBytes];
  __bf16* Hs = reinterpret_cast<__bf16*>(smem);                  // h2 / dh2
  float* Hd = reinterpret_cast<float*>(smem + kTileBytes);       // head
  __bf16* Ds = reinterpret_cast<__bf16*>(smem + kTileBytes + kHdBytes);

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row_a = lane & 15;
  const int kseg = lane >> 4;
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;

  const int slab = blockIdx.x;
  const int m_per_slab = (M + slabs - 1) / slabs;
  const int m_begin = slab * m_per_slab;
  const int m_end = min(M, m_begin + m_per_slab);
  const int nrows = max(0, m_end - m_begin);        // <= kHlbRows (launcher)
  const int rpad = min(kHlbRows, (nrows + 31) & ~31);  // rows the MFMAs touch
  const int n_actions = head_dim - 1;

  // ---- stage ----------------------------------------------------------
  // W3t fragments for the head GEMM: B[k][col] = W3t[col][k], zero columns
  // past head_dim (what the GEMM's guarded staging puts in its tile)
  bf16x8 bh[kHlbHid / 32];
#pragma unroll
  for (int ks = 0; ks < kHlbHid / 32; ++ks) {
    bh[ks] = bf16x8{};
    if (row_a < head_dim)
      bh[ks] = *reinterpret_cast<const bf16x8*>(
          &W3t[row_a * kHlbHid + ks * 32 + kseg * 8]);
  }
  // dhead image: zero everywhere the loss does not write (k/n padding of
  // the MFMA operands, rows past the slab end)
  *reinterpret_cast<bf16x8*>(&Ds[tid * 8]) = bf16x8{};
  if (nrows == kHlbRows) {
    // 64 KB = 64 glds instructions of 1 KB, 16 per wave
    for (int j = 0; j < 16; ++j) {
      const int e0 = (wave * 16 + j) * 512;
      const int e = e0 + lane * 8;
      const int r = e >> 8;
      const int p = (e >> 3) & 31;
      const int c = (p & 16) | ((p ^ r) & 15);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &h2[(int64_t)(m_begin + r) * kHlbHid + c * 8]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(Hs + e0), 16, 0,
          0);
    }
  } else {
    for (int idx = tid; idx < rpad * 32; idx += 256) {
      const int r = idx >> 5;
      const int p = idx & 31;
      const int c = (p & 16) | ((p ^ r) & 15);
      bf16x8 v = bf16x8{};
      if (r < nrows)
        v = *reinterpret_cast<const bf16x8*>(
            &h2[(int64_t)(m_begin + r) * kHlbHid + c * 8]);
      *reinterpret_cast<bf16x8*>(&Hs[idx * 8]) = v;
    }
  }
  __syncthreads();  // vmcnt(0) inside the barrier drains the glds

  // ---- head = h2 @ W3t^T + b3 (wave w: rows w*32 .. w*32+31) ------------
  if (wave * 32 < rpad) {
    for (int mi = 0; mi < 2; ++mi) {
      const int r0 = wave * 32 + mi * 16;
      f32x4 acc = {};
#pragma unroll
      for (int ks = 0; ks < kHlbHid / 32; ++ks) {  // sequential k order
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(
            &Hs[hlb_off(r0 + row_a, ks * 32 + kseg * 8)]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bh[ks], acc, 0, 0, 0);
      }
      if (ccol < head_dim) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[r];
          v += b3[ccol];
          Hd[(r0 + crow_base + r) * kHlbHdLd + ccol] = v;
        }
      }
    }
  }
  __syncthreads();

  // ---- loss backward: one thread per row -------------------------------
  {
    float l_pi = 0.f, l_v = 0.f, l_ent = 0.f, l_kl = 0.f, l_clip = 0.f;
    if (tid < nrows) {
      const int m = m_begin + tid;
      ppo_loss_row(Hd + tid * kHlbHdLd, Ds + tid * kHlbHead, (int)actions[m],
                   old_logp[m], adv[m], ret[m], n_actions, clip_eps, ent_coef,
                   vf_coef, inv_count, l_pi, l_v, l_ent, l_kl, l_clip);
    }
    // logging sums: wave shuffle reduce, one atomicAdd per stat per wave,
    // into accumulator row slab % loss_shards (rows kLossShardLd floats
    // apart).  Device-scope float atomics on ONE cache line retire at about
    // 88 per us whatever the word, so the 5120 of a 512-block launch on a
    // single [5] accumulator take 58 us; spread over 64 lines they are free.
    if (losses && wave * 64 < nrows) {
      losses += (slab % loss_shards) * kLossShardLd;
      float vals[5] = {l_pi, l_v, l_ent, l_kl, l_clip};
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        float x = vals[s];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) atomicAdd(&losses[s], x * inv_count);
      }
    }
  }
  __syncthreads();

  // ---- head / dhead out (the slab's rows are contiguous in both) --------
  for (int idx = tid; idx < nrows * head_dim; idx += 256) {
    const int r = idx / head_dim;
    const int j = idx - r * head_dim;
    head[(int64_t)m_begin * head_dim + idx] = Hd[r * kHlbHdLd + j];
    dhead[(int64_t)m_begin * head_dim + idx] = Ds[r * kHlbHead + j];
  }

  // W3 fragments for the dgrad: B[k][n] = W3[n][k], k < head_dim
  // (wave w: columns w*64 .. w*64+63)
  bf16x8 bw[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bw[g] = bf16x8{};
    const int n = (wave * 4 + g) * 16 + row_a;
    // every load issued (index clamped in bounds), then masked: a branch
    // around each load would wait for them one by one
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kseg * 8 + i;
      const __bf16 w = W3[n * head_dim + min(k, head_dim - 1)];
      bw[g][i] = (k < head_dim) ? w : (__bf16)0.f;
    }
  }

  // ---- W3 / b3 slab partials (wave w: dW rows w*64 .. w*64+63) ----------
  {
    const int nchunks = (nrows + 31) / 32;
    f32x4 acc[4] = {};
    for (int ci = 0; ci < nchunks; ++ci) {
      const int m0 = ci * 32 + kseg * 8;  // reduction index kseg*8+i
      bf16x8 bf_;
#pragma unroll
      for (int i = 0; i < 8; ++i) bf_[i] = Ds[(m0 + i) * kHlbHead + row_a];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        bf16x8 af;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[i] = Hs[hlb_off(m0 + i, (wave * 4 + f) * 16 + row_a)];
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf_, acc[f], 0, 0,
                                                         0);
      }
    }
    float* out = dW_part + (int64_t)slab * kHlbHid * head_dim;
    if (ccol < head_dim) {
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int grow = (wave * 4 + f) * 16 + crow_base + r;
          out[grow * head_dim + ccol] = acc[f][r];
        }
    }
    if (tid < head_dim) {
      float db_acc = 0.f;
      for (int ci = 0; ci < nchunks; ++ci) {
        // row order, as wgrad_partial_kernel sums it; rows past the slab
        // end are zero in Ds, and s + 0.f leaves s (never -0.f: it starts
        // at +0.f) as it is, so the chunk is read whole, loads first
        float x[32];
#pragma unroll
        for (int i = 0; i < 32; ++i)
          x[i] = bf2f(Ds[(ci * 32 + i) * kHlbHead + tid]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) s += x[i];
        db_acc += s;
      }
      db_part[(int64_t)slab * head_dim + tid] = db_acc;
    }
  }
  __syncthreads();  // every h2 read of the wgrad is done: dh2 may overwrite

  // ---- dh2 = dhead @ W3^T * (1 - h2^2), written over the h2 tile --------
  // The MFMA computes the TRANSPOSED fragment (W3 as the A operand, dhead
  // as B: the same products at the same k positions), so a lane holds four
  // consecutive columns of one row and the epilogue moves 8 B per LDS access
  // instead of 2.
  for (int mi = 0; mi < rpad / 16; ++mi) {
    bf16x8 df = bf16x8{};
    if (kseg < kHlbHead / 8)
      df = *reinterpret_cast<const bf16x8*>(
          &Ds[(mi * 16 + row_a) * kHlbHead + kseg * 8]);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          bw[g], df, f32x4{}, 0, 0, 0);
      // acc[r]: column (wave*4+g)*16 + crow_base + r of row mi*16 + ccol
      bf16x4* yp = reinterpret_cast<bf16x4*>(
          &Hs[hlb_off(mi * 16 + ccol, (wave * 4 + g) * 16 + crow_base)]);
      const bf16x4 yv = *yp;
      bf16x4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[r];
        float y = bf2f(yv[r]);
        v *= (1.f - y * y);
        ov[r] = f2bf(v);
      }
      *yp = ov;
    }
  }
  __syncthreads();

  for (int idx = tid; idx < nrows * 32; idx += 256) {
    const int r = idx >> 5;
    const int p = idx & 31;
    const int c = (p & 16) | ((p ^ r) & 15);
    *reinterpret_cast<bf16x8*>(&dh2[(int64_t)(m_begin + r) * kHlbHid + c * 8]) =
        *reinterpret_cast<const bf16x8*>(&Hs[idx * 8]);
  }
}

// normalize advantages in-place: (a - mean) / (std + 1e-8), deterministic
__global__ void adv_norm_stats_kernel(const float* __restrict__ adv, int64_t n,
                                      float* __restrict__ part /*[blocks*2]*/) {
  __shared__ float red[512];
  float s = 0.f, ss = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    s += adv[i];
    ss += adv[i] * adv[i];
  }
  red[threadIdx.x] = s;
  red[256 + threadIdx.x] = ss;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      red[256 + threadIdx.x] += red[256 + threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x] = red[0];
    part[gridDim.x + blockIdx.x] = red[256];
  }
}

__global__ void adv_norm_apply_kernel(float* __restrict__ adv, int64_t n,
                                      const float* __restrict__ part,
                                      int nparts) {
  __shared__ float mean_s, inv_std_s;
  if (threadIdx.x == 0) {
    float s = 0.f, ss = 0.f;
    for (int i = 0; i < nparts; ++i) { s += part[i]; ss += part[nparts + i]; }
    const float mean = s / (float)n;
    float var = ss / (float)n - mean * mean;
    var = fmaxf(var, 0.f);
    mean_s = mean;
    inv_std_s = 1.f / (sqrtf(var) + 1e-8f);
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    adv[i] = (adv[i] - mean_s) * inv_std_s;
}

// ---------------------------------------------------------------------------
// LSTM cell, elementwise over [M, H] (the GEMM part — x@Wx + h@Wh + b — runs
// on the MFMA GEMM above; these kernels do the gate math).
// Gate layout in gates_pre [M, 4H]: [i | f | g | o].
//   c_new = sig(f)*c_prev + sig(i)*tanh(g);  h_new = sig(o)*tanh(c_new)
// fwd keeps gates_pre and c_prev/c_new around so bwd can recompute the
// activations (cheaper than storing five activation planes).
// ---------------------------------------------------------------------------
GFX_DEV float fast_sigmoid(float x) {
  x = fminf(fmaxf(x, -30.f), 30.f);
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f));
}

// Gate layout is INTERLEAVED along the 4H axis (models/lstm.py): column
// 4*k + g holds gate g of hidden unit k (g: 0=i 1=f 2=g~ 3=o), so every
// per-unit gate access is ONE contiguous vector load (f32x4 / bf16x4)
// instead of four reads H apart.
//
// gates_h (optional, bf16): the recurrent projection h@Wh kept as a
// SEPARATE bf16 tensor and summed here — the fused alternative (f32
// accumulate-GEMM into gates_pre) read-modify-writes a 4x bigger buffer
// and was the dominant BPTT kernel.
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// 4-wide interleaved gate pre-activations of hidden unit k for row m
// (gates_pre is bf16 like gates_h; the sum runs in f32)
GFX_DEV f32x4 gate_pre4(const __bf16* __restrict__ gates_pre,
                        const __bf16* __restrict__ gates_h, int64_t idx4) {
  const bf16x4 gx = *reinterpret_cast<const bf16x4*>(&gates_pre[idx4]);
  f32x4 v;
  for (int j = 0; j < 4; ++j) v[j] = bf2f(gx[j]);
  if (gates_h) {
    const bf16x4 gh = *reinterpret_cast<const bf16x4*>(&gates_h[idx4]);
    for (int j = 0; j < 4; ++j) v[j] += bf2f(gh[j]);
  }
  return v;
}

// Cell forward math shared by the standalone cell kernel AND the fused
// GEMM epilogue: explicit fmaf pins the contraction so both compile to
// the same instruction sequence (a 1-ulp fma-vs-mul+add divergence
// between the two kernels broke bitwise fused==unfused once).
GFX_DEV void lstm_cell_math(const f32x4 gp, float cp, float* c_out,
                            float* h_out, bf16x4* acts_out) {
// contraction off: the compiler must not fuse mul+add differently in the
// different kernels that inline this helper (bitwise fused==unfused);
// the one fma we DO want is written explicitly below
#pragma clang fp contract(off)
  const float i = fast_sigmoid(gp[0]);
  const float f = fast_sigmoid(gp[1]);
  const float g = fast_tanh(gp[2]);
  const float o = fast_sigmoid(gp[3]);
  const float c = __builtin_fmaf(f, cp, i * g);
  *c_out = c;
  *h_out = o * fast_tanh(c);
  if (acts_out) {
    (*acts_out)[0] = f2bf(i);
    (*acts_out)[1] = f2bf(f);
    (*acts_out)[2] = f2bf(g);
    (*acts_out)[3] = f2bf(o);
  }
}


// Cell backward math shared by the standalone bwd kernel and the fused
// bwd kernel (same contraction-pinning rationale as lstm_cell_math).
// The four gate ACTIVATIONS arrive as saved bf16 (written by the forward
// cell) — the backward no longer touches gates_pre/gates_h at all, which
// removes 268 MB/minibatch of reads and all transcendental recompute.
// dh_next/dc_next arrive PRE-masked (0 when absent or across a reset).
GFX_DEV void lstm_cell_bwd_math(const bf16x4 acts, float cp, float c,
                                float dh_head_v, float dh_next_v,
                                float dc_next_v, bf16x4* dg, float* dcp) {
#pragma clang fp contract(off)
  const float i = bf2f(acts[0]);
  const float f = bf2f(acts[1]);
  const float g = bf2f(acts[2]);
  const float o = bf2f(acts[3]);
  const float tc = fast_tanh(c);
  const float dhv = dh_head_v + dh_next_v;
  float dc = dhv * o * (1.f - tc * tc);
  dc += dc_next_v;
  (*dg)[0] = f2bf(dc * g * i * (1.f - i));
  (*dg)[1] = f2bf(dc * cp * f * (1.f - f));
  (*dg)[2] = f2bf(dc * i * (1.f - g * g));
  (*dg)[3] = f2bf(dhv * tc * o * (1.f - o));
  *dcp = dc * f;
}

__global__ void lstm_cell_fwd_kernel(
    const __bf16* __restrict__ gates_pre,  // [M, 4H] (x-projection + bias)
    const __bf16* __restrict__ gates_h,   // [M, 4H] or null (h-projection)
    const float* __restrict__ c_prev,     // [M, H]
    float* __restrict__ c_new,            // [M, H]
    __bf16* __restrict__ h_new,           // [M, H] (bf16: feeds next GEMM)
    const bool* __restrict__ done,        // [M] or null: also emit the
    __bf16* __restrict__ h_masked,        //   reset-masked state that feeds
    float* __restrict__ c_masked,         //   the NEXT step (one fewer
    __bf16* __restrict__ acts_out,        // [M, 4H] saved activations or null
    int64_t M, int H) {                   //   launch than masked_state)
  const int64_t total = M * H;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = idx / H;
    const f32x4 gp = gate_pre4(gates_pre, gates_h, idx * 4);
    float c, hval;
    bf16x4 av;
    lstm_cell_math(gp, c_prev[idx], &c, &hval, acts_out ? &av : nullptr);
    if (acts_out) *reinterpret_cast<bf16x4*>(&acts_out[idx * 4]) = av;
    c_new[idx] = c;
    const __bf16 hb = f2bf(hval);
    h_new[idx] = hb;
    if (done) {
      const bool d = done[m];
      h_masked[idx] = d ? (__bf16)0.f : hb;
      c_masked[idx] = d ? 0.f : c;
    }
  }
}

// dh_head: gradient from the policy/value head (w.r.t. the RAW h output of
// this step).  dh_next: gradient arriving from step l+1's recurrent GEMM
// (w.r.t. the MASKED h input of step l+1) — masked by `done` (the episode
// boundary AFTER this step) along with dc_next, so no gradient crosses a
// reset.
__global__ void lstm_cell_bwd_kernel(
    const __bf16* __restrict__ acts,      // [M, 4H] saved activations
    const float* __restrict__ c_prev,     // [M, H] (masked input c)
    const float* __restrict__ c_new,      // [M, H] (raw output c)
    const __bf16* __restrict__ dh_head,   // [M, H] (head-dgrad slab, bf16)
    const float* __restrict__ dh_next,    // [M, H] or null
    const float* __restrict__ dc_next,    // [M, H] or null (last step)
    const bool* __restrict__ done,        // [M] or null
    __bf16* __restrict__ dgates,          // [M, 4H] out (bf16: feeds wgrad)
    float* __restrict__ dc_prev,          // [M, H] out
    int64_t M, int H) {
  // one thread owns FOUR consecutive hidden units: acts/dgates move as
  // bf16x8 pairs, the f32 streams as f32x4 (H % 4 == 0 enforced by the
  // binding) — the scalar-per-unit version ran at half its traffic floor
  const int64_t groups = M * (H / 4);
  for (int64_t gidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       gidx < groups; gidx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = gidx / (H / 4);
    const int64_t idx0 = gidx * 4;  // == m * H + u0
    const float mask = (done && done[m]) ? 0.f : 1.f;
    const f32x4 cp = *reinterpret_cast<const f32x4*>(&c_prev[idx0]);
    const f32x4 cn = *reinterpret_cast<const f32x4*>(&c_new[idx0]);
    const bf16x4 dhb = *reinterpret_cast<const bf16x4*>(&dh_head[idx0]);
    f32x4 dhh;
    for (int j = 0; j < 4; ++j) dhh[j] = bf2f(dhb[j]);
    f32x4 dhn = {}, dcn = {};
    if (dh_next) dhn = *reinterpret_cast<const f32x4*>(&dh_next[idx0]);
    if (dc_next) dcn = *reinterpret_cast<const f32x4*>(&dc_next[idx0]);
    bf16x4 dg4[4];
    f32x4 dcp4;
    for (int j = 0; j < 4; ++j) {
      const bf16x4 av = *reinterpret_cast<const bf16x4*>(
          &acts[(idx0 + j) * 4]);
      float dcp;
      lstm_cell_bwd_math(av, cp[j], cn[j], dhh[j],
                         dh_next ? mask * dhn[j] : 0.f,
                         dc_next ? mask * dcn[j] : 0.f, &dg4[j], &dcp);
      dcp4[j] = dcp;
    }
    *reinterpret_cast<bf16x8*>(&dgates[idx0 * 4]) =
        *reinterpret_cast<const bf16x8*>(&dg4[0]);
    *reinterpret_cast<bf16x8*>(&dgates[idx0 * 4 + 8]) =
        *reinterpret_cast<const bf16x8*>(&dg4[2]);
    *reinterpret_cast<f32x4*>(&dc_prev[idx0]) = dcp4;
  }
}

// ---------------------------------------------------------------------------
// FUSED recurrent step: gates_h = h_in @ Wh^T computed by the standard MFMA
// pipeline (TRANS_B, NFRAG=2, 64x64 tile — same staging/double-buffering as
// gemm_kernel), with the LSTM CELL as the epilogue.  The interleaved gate
// layout makes each 64-column output tile hold 16 COMPLETE hidden units, so
// the cell needs no cross-tile exchange: accumulators go to an LDS tile,
// one barrier, then each thread does the gate math for 4 (row, unit) pairs.
// Removes the separate cell launch from the latency-bound sequential chain
// (profiles/lstm_kernel_stats_r2.txt: cell_fwd 11.3 us x 512/update).
//
// Bitwise parity with the unfused pair: the GEMM result is rounded to bf16
// BEFORE the gate sum (matching the bf16 gates_h tensor of the unfused
// path) and the MFMA K-chunk order is identical.
// ---------------------------------------------------------------------------
template <bool WRITE_GH>
__global__ __launch_bounds__(256, 2) void lstm_gemm_cell_fwd_kernel(
    const __bf16* __restrict__ A,         // h_in [M, K=H]
    const __bf16* __restrict__ B,         // Wh^T [N=4H, K=H]
    const __bf16* __restrict__ gates_pre,  // [M, 4H] (x-proj + bias)
    __bf16* __restrict__ acts_out,        // [M, 4H] saved activations (if WRITE_GH)
    const float* __restrict__ c_prev,     // [M, H]
    float* __restrict__ c_new,            // [M, H]
    __bf16* __restrict__ h_new,           // [M, H]
    const bool* __restrict__ done,        // [M] or null
    __bf16* __restrict__ h_masked,        // [M, H] (if done)
    float* __restrict__ c_masked,         // [M, H] (if done)
    int M, int N, int K) {
  constexpr int BM = 64, BK = 32, BN = 64;
  constexpr int LDA = BK;  // TRANS_B images are unpadded linear (glds)
  __shared__ __align__(16) __bf16 As[2][BM][LDA];
  __shared__ __align__(16) __bf16 Bs[2][BN][BK];
  __shared__ float Cs[BM][BN + 1];  // accum tile for the cell phase

  const int bm = blockIdx.x * BM;
  const int bn = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wr = wave >> 1;
  const int wc = wave & 1;

  f32x4 acc[2][2] = {};
  const int row_a = lane & 15;
  const int kseg = lane >> 4;
  const int a_r = tid >> 2;
  const int a_c8 = (tid & 3) * 8;

  bf16x8 ra, rb;
  auto load_tile = [&](int k0) {
    ra = bf16x8{};
    const int gr = bm + a_r;
    if (gr < M) {
      const int gk = k0 + a_c8;
      if (gk + 8 <= K) {
        ra = *reinterpret_cast<const bf16x8*>(&A[(int64_t)gr * K + gk]);
      } else {
        for (int i = 0; i < 8; ++i)
          ra[i] = (gk + i < K) ? A[(int64_t)gr * K + gk + i] : (__bf16)0.f;
      }
    }
    rb = bf16x8{};
    const int gn = bn + a_r;  // BN == BM: same staging coordinates
    if (gn < N) {
      const int gk = k0 + a_c8;
      if (gk + 8 <= K) {
        rb = *reinterpret_cast<const bf16x8*>(&B[(int64_t)gn * K + gk]);
      } else {
        for (int i = 0; i < 8; ++i)
          rb[i] = (gk + i < K) ? B[(int64_t)gn * K + gk + i] : (__bf16)0.f;
      }
    }
  };
  auto store_tile = [&](int buf) {
    *reinterpret_cast<bf16x8*>(&As[buf][a_r][a_c8]) = ra;
    *reinterpret_cast<bf16x8*>(&Bs[buf][a_r][a_c8]) = rb;
  };
  const bool can_glds = (bm + BM <= M) && (bn + BN <= N);
  auto glds_tile = [&](int buf, int k0) {
    {
      const int e0 = wave * 512;
      const int row = (e0 + lane * 8) / BK;
      const int col = (e0 + lane * 8) % BK;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &A[(int64_t)(bm + row) * K + k0 + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &As[buf][0][0] + e0),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(uintptr_t)(
              &B[(int64_t)(bn + row) * K + k0 + col]),
          (__attribute__((address_space(3))) void*)(uintptr_t)(
              &Bs[buf][0][0] + e0),
          16, 0, 0);
    }
  };
  auto stage = [&](int buf, int k0) {
    if (can_glds && k0 + BK <= K) {
      glds_tile(buf, k0);
    } else {
      load_tile(k0);
      store_tile(buf);
    }
  };

  const int ktiles = (K + BK - 1) / BK;
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const int cur = kt & 1;
    const bool nxt_glds = kt + 1 < ktiles && can_glds && (kt + 1) * BK + BK <= K;
    if (nxt_glds) glds_tile(1 - cur, (kt + 1) * BK);
    else if (kt + 1 < ktiles) load_tile((kt + 1) * BK);

    bf16x8 af[2], bf[2];
    for (int mi = 0; mi < 2; ++mi)
      af[mi] = *reinterpret_cast<const bf16x8*>(
          &As[cur][wr * 32 + mi * 16 + row_a][kseg * 8]);
    for (int ni = 0; ni < 2; ++ni)
      bf[ni] = *reinterpret_cast<const bf16x8*>(
          &Bs[cur][wc * 32 + ni * 16 + row_a][kseg * 8]);
    for (int mi = 0; mi < 2; ++mi)
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);

    if (kt + 1 < ktiles && !nxt_glds) store_tile(1 - cur);
    __syncthreads();
  }

  // accumulators -> LDS tile (bf16-round to match the unfused gates_h)
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < 2; ++ni)
      for (int r = 0; r < 4; ++r)
        Cs[wr * 32 + mi * 16 + crow_base + r][wc * 32 + ni * 16 + ccol] =
            bf2f(f2bf(acc[mi][ni][r]));
  __syncthreads();

  // ---- cell phase: one thread owns FOUR CONSECUTIVE units of one row
  // (4 threads/row x 64 rows), so every global access is a vector op:
  // gates/acts 32 B, c 16 B f32x4, h 8 B bf16x4.  (The first mapping —
  // 4 rows x 1 unit per thread — emitted 20 scattered scalar stores.)
  const int rl = tid >> 2;            // local row 0..63
  const int u0l = (tid & 3) * 4;      // first local unit (of 16)
  const int H = N / 4;
  const int grow = bm + rl;
  if (grow < M) {
    const int64_t idx0 = (int64_t)grow * H + (bn / 4 + u0l);
    const int64_t g0 = (int64_t)grow * N + (int64_t)(bn + u0l * 4);
    float c4[4], h4[4];
    bf16x4 av4[4];
    for (int j = 0; j < 4; ++j) {
      f32x4 gp;
      const bf16x4 gxb = *reinterpret_cast<const bf16x4*>(
          &gates_pre[g0 + j * 4]);
      for (int q = 0; q < 4; ++q)
        gp[q] = bf2f(gxb[q]) + Cs[rl][(u0l + j) * 4 + q];
      lstm_cell_math(gp, c_prev[idx0 + j], &c4[j], &h4[j],
                     WRITE_GH ? &av4[j] : nullptr);
    }
    if (WRITE_GH) {
      *reinterpret_cast<bf16x8*>(&acts_out[g0]) =
          *reinterpret_cast<const bf16x8*>(&av4[0]);
      *reinterpret_cast<bf16x8*>(&acts_out[g0 + 8]) =
          *reinterpret_cast<const bf16x8*>(&av4[2]);
    }
    f32x4 cv;
    bf16x4 hv;
    for (int j = 0; j < 4; ++j) {
      cv[j] = c4[j];
      hv[j] = f2bf(h4[j]);
    }
    *reinterpret_cast<f32x4*>(&c_new[idx0]) = cv;
    *reinterpret_cast<bf16x4*>(&h_new[idx0]) = hv;
    if (done) {
      const bool d = done[grow];
      f32x4 cm;
      bf16x4 hm;
      for (int j = 0; j < 4; ++j) {
        cm[j] = d ? 0.f : cv[j];
        hm[j] = d ? (__bf16)0.f : hv[j];
      }
      *reinterpret_cast<f32x4*>(&c_masked[idx0]) = cm;
      *reinterpret_cast<bf16x4*>(&h_masked[idx0]) = hm;
    }
  }
}

// ---------------------------------------------------------------------------
// FUSED BPTT backward step, tile-parallel: the cell backward (dgates) and
// the recurrent dgrad GEMM dh_prev = dgates @ Wh^T in ONE kernel with the
// standard 64x64 output tiling — each (bm, bn) block COMPUTES its A tile
// (dgates chunk) on the fly instead of reading a materialized tensor.
// The cell math is recomputed by each of the H/64 bn-blocks (the gate
// slabs are LLC-resident, the transcendentals are cheap), and only the
// bn==0 block writes dgates/dc_prev to global.  v1 of this fusion was a
// 16-row slab across the full 4H width: 4x the Wh traffic of this tiling
// and 1 workgroup/CU — measured SLOWER than the unfused pair
// (profiles/PERF_NOTES.md).  Bitwise parity: dgates are bf16-rounded
// before the MFMA, shared lstm_cell_bwd_math, gemm-identical K order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void lstm_bwd_fused_kernel(
    const __bf16* __restrict__ acts,       // [M, 4H] saved activations
    const float* __restrict__ c_prev,      // [M, H]
    const float* __restrict__ c_new,       // [M, H]
    const __bf16* __restrict__ dh_head,    // [M, H] (bf16 head-dgrad slab)
    const float* __restrict__ dh_next,     // [M, H] or null
    const float* __restrict__ dc_next,     // [M, H] or null
    const bool* __restrict__ done,         // [M] or null
    const __bf16* __restrict__ B,          // Wh [N=H, K=4H] (trans_b layout)
    __bf16* __restrict__ dgates,           // [M, 4H] out
    float* __restrict__ dc_prev,           // [M, H] out
    float* __restrict__ dh_prev,           // [M, H] out, or null (step 0)
    int M, int H) {
  constexpr int BM = 64, BK = 32, BN = 64;
  const int K = 4 * H;
  const int N = H;
  __shared__ __align__(16) __bf16 As[2][BM][BK];
  __shared__ __align__(16) __bf16 Bs[2][BN][BK];

  const int bm = blockIdx.x * BM;
  const int bn = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wr = wave >> 1;
  const int wc = wave & 1;
  const bool write_dg = blockIdx.y == 0;

  // compute the dgates chunk for units [kt*8, kt*8+8) of rows [bm, bm+64)
  auto compute_a = [&](int buf, int kt) {
    const int u0 = kt * 8;
    for (int j = 0; j < 2; ++j) {
      const int p = tid + j * 256;       // (row, unit) pair
      const int rl = p >> 3;
      const int ul = p & 7;
      const int grow = bm + rl;
      bf16x4 dg = {};
      float dcp = 0.f;
      if (grow < M) {
        const int64_t idx = (int64_t)grow * H + (u0 + ul);
        const float mask = (done && done[grow]) ? 0.f : 1.f;
        const bf16x4 av = *reinterpret_cast<const bf16x4*>(&acts[idx * 4]);
        lstm_cell_bwd_math(av, c_prev[idx], c_new[idx], bf2f(dh_head[idx]),
                           dh_next ? mask * dh_next[idx] : 0.f,
                           dc_next ? mask * dc_next[idx] : 0.f, &dg, &dcp);
        if (write_dg) {
          *reinterpret_cast<bf16x4*>(&dgates[idx * 4]) = dg;
          dc_prev[idx] = dcp;
        }
      }
      *reinterpret_cast<bf16x4*>(&As[buf][rl][ul * 4]) = dg;
    }
  };
  if (dh_prev == nullptr) {
    // step 0: no recurrent-grad consumer — cell backward only (bn==0 grid)
    const int ktiles = K / BK;
    for (int kt = 0; kt < ktiles; ++kt) compute_a(0, kt);
    return;
  }
  auto glds_b = [&](int buf, int k0) {
    const int e0 = wave * 512;  // BN*BK = 2048 elems = 4 waves x 512
    const int row = (e0 + lane * 8) / BK;
    const int col = (e0 + lane * 8) % BK;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(uintptr_t)(
            &B[(int64_t)(bn + row) * K + k0 + col]),
        (__attribute__((address_space(3))) void*)(uintptr_t)(
            &Bs[buf][0][0] + e0),
        16, 0, 0);
  };

  f32x4 acc[2][2] = {};
  const int row_a = lane & 15;
  const int kseg = lane >> 4;
  const int ktiles = K / BK;
  glds_b(0, 0);
  compute_a(0, 0);
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ktiles) {
      glds_b(1 - cur, (kt + 1) * BK);
      compute_a(1 - cur, kt + 1);
    }
    bf16x8 af[2], bf[2];
    for (int mi = 0; mi < 2; ++mi)
      af[mi] = *reinterpret_cast<const bf16x8*>(
          &As[cur][wr * 32 + mi * 16 + row_a][kseg * 8]);
    for (int ni = 0; ni < 2; ++ni)
      bf[ni] = *reinterpret_cast<const bf16x8*>(
          &Bs[cur][wc * 32 + ni * 16 + row_a][kseg * 8]);
    for (int mi = 0; mi < 2; ++mi)
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    __syncthreads();
  }
  const int crow = (lane >> 4) * 4;
  const int ccol = lane & 15;
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < 2; ++ni) {
      const int gcol = bn + wc * 32 + ni * 16 + ccol;
      for (int r = 0; r < 4; ++r) {
        const int grow = bm + wr * 32 + mi * 16 + crow + r;
        if (grow < M && gcol < N)
          dh_prev[(int64_t)grow * N + gcol] = acc[mi][ni][r];
      }
    }
}

// zero the recurrent state of terminated envs (rollout path: applied right
// after the fused env step, so the next policy step starts fresh)
__global__ void mask_reset_kernel(__bf16* __restrict__ h,
                                  float* __restrict__ c,
                                  const bool* __restrict__ done, int64_t M,
                                  int H) {
  const int64_t total = M * H;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    if (done[idx / H]) {
      h[idx] = (__bf16)0.f;
      c[idx] = 0.f;
    }
  }
}

// masked copy: out = in * (1 - done)  (BPTT fwd: the h/c INPUT of step l+1)
__global__ void masked_state_kernel(const __bf16* __restrict__ h_raw,
                                    const float* __restrict__ c_raw,
                                    const bool* __restrict__ done,
                                    __bf16* __restrict__ h_in,
                                    float* __restrict__ c_in, int64_t M,
                                    int H) {
  const int64_t total = M * H;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const bool d = done[idx / H];
    h_in[idx] = d ? (__bf16)0.f : h_raw[idx];
    c_in[idx] = d ? 0.f : c_raw[idx];
  }
}

// ---------------------------------------------------------------------------
// Fused MLP policy rollout step: obs -> tanh(obs@W1+b1) -> tanh(.@W2+b2)
// -> head(.@W3+b3) -> categorical sample, ONE kernel.
//
// The unfused rollout chain (3 GEMMs + sampler) is execution-floor bound
// (~8-10us per kernel at N=4096 regardless of bytes); fusing removes three
// kernel floors per env step (x128 steps per update).  The math replicates
// the GEMM kernel exactly (same BK=32 chunking, same MFMA sequence, bias
// added in f32, tanh via fast_tanh, h1/h2 rounded to bf16 between layers),
// so outputs are BITWISE identical to the unfused path — asserted by
// tests/test_gpu_trainer.py::test_fused_rollout_equals_unfused.
//
// Shapes: H = 256 (4 waves each own 32 rows x 128 cols), head_dim <= 16,
// D (obs_dim) arbitrary.  Block = 256 threads = 64 env rows; weights are
// the transposed mirrors (W1t [256, D], W2t [256, 256], W3t [A+1, 256]).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void mlp_policy_rollout_kernel(
    const __bf16* __restrict__ obs,   // [N, D]
    const __bf16* __restrict__ W1t,   // [256, D]
    const float* __restrict__ b1,     // [256]
    const __bf16* __restrict__ W2t,   // [256, 256]
    const float* __restrict__ b2,     // [256]
    const __bf16* __restrict__ W3t,   // [head_dim, 256]
    const float* __restrict__ b3,     // [head_dim]
    int64_t* __restrict__ actions, float* __restrict__ logp,
    float* __restrict__ value, int N, int D, int n_actions, uint64_t seed,
    uint64_t step, const unsigned long long* __restrict__ step_base,
    int row_offset, int greedy) {
  constexpr int BM = 64, BK = 32, H = 256;
  constexpr int LDT = BK + 8;     // staged-operand row (bf16)
  constexpr int LDH = H + 8;      // h1/h2 image row (bf16)
  __shared__ __bf16 As[2][BM][LDT];
  __shared__ __bf16 Bs[2][H][LDT];       // weight tile [n][k]
  __shared__ __bf16 Himg[2][BM][LDH];    // h1 / h2 images
  __shared__ float Head[BM][20];         // head values (row pad: 20 f32)
  const int bm = blockIdx.x * BM;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int row_a = lane & 15;
  const int kseg = lane >> 4;
  const int a_r = tid >> 2, a_c8 = (tid & 3) * 8;
  const int b_r = tid >> 2, b_c8 = (tid & 3) * 8;
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  f32x4 acc[2][8];
  bf16x8 ra, rb[4];

  // ONE shared dense-layer loop (layer selected at runtime): the first
  // version macro-duplicated the whole GEMM body per layer and the
  // allocator thrashed (~2.5k SGPR spills).  Math is bitwise identical to
  // the unfused GEMM kernel (same BK chunking, MFMA order, f32 bias,
  // fast_tanh, bf16 rounding).
  for (int layer = 0; layer < 2; ++layer) {
    const bool from_global = layer == 0;
    const __bf16* Wt = from_global ? W1t : W2t;
    const float* bias = from_global ? b1 : b2;
    const int K = from_global ? D : H;
    const __bf16(*Ximg)[LDH] = Himg[0];
    __bf16(*Yimg)[LDH] = Himg[layer];
    const int ktiles = (K + BK - 1) / BK;
    for (int mi = 0; mi < 2; ++mi)
      for (int ni = 0; ni < 8; ++ni) acc[mi][ni] = f32x4{};
    for (int kt = -1; kt + 1 < ktiles + 1; ++kt) {
      // stage chunk kt+1 (kt==-1 is the prologue), compute chunk kt
      const int knext = (kt + 1) * BK;
      if (kt + 1 < ktiles) {
        if (from_global) {
          ra = bf16x8{};
          const int gr = bm + a_r;
          if (gr < N) {
            const int gk = knext + a_c8;
            if (gk + 8 <= K) {
              ra = *reinterpret_cast<const bf16x8*>(&obs[(int64_t)gr * D + gk]);
            } else {
              for (int i = 0; i < 8; ++i)
                ra[i] = (gk + i < K) ? obs[(int64_t)gr * D + gk + i]
                                     : (__bf16)0.f;
            }
          }
        } else {
          ra = *reinterpret_cast<const bf16x8*>(&Ximg[a_r][knext + a_c8]);
        }
        for (int j = 0; j < 4; ++j) {
          const int gn = b_r + j * 64;
          const int gk = knext + b_c8;
          if (gk + 8 <= K) {
            rb[j] = *reinterpret_cast<const bf16x8*>(&Wt[(int64_t)gn * K + gk]);
          } else {
            rb[j] = bf16x8{};
            for (int i = 0; i < 8; ++i)
              rb[j][i] = (gk + i < K) ? Wt[(int64_t)gn * K + gk + i]
                                      : (__bf16)0.f;
          }
        }
      }
      if (kt >= 0) {
        const int cur = kt & 1;
        bf16x8 af[2], bf[8];
        for (int mi = 0; mi < 2; ++mi)
          af[mi] = *reinterpret_cast<const bf16x8*>(
              &As[cur][wr * 32 + mi * 16 + row_a][kseg * 8]);
        for (int ni = 0; ni < 8; ++ni)
          bf[ni] = *reinterpret_cast<const bf16x8*>(
              &Bs[cur][wc * 128 + ni * 16 + row_a][kseg * 8]);
        for (int mi = 0; mi < 2; ++mi)
          for (int ni = 0; ni < 8; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
      }
      if (kt + 1 < ktiles) {
        const int nxt = (kt + 1) & 1;
        *reinterpret_cast<bf16x8*>(&As[nxt][a_r][a_c8]) = ra;
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<bf16x8*>(&Bs[nxt][b_r + j * 64][b_c8]) = rb[j];
      }
      __syncthreads();
    }
    for (int mi = 0; mi < 2; ++mi)
      for (int ni = 0; ni < 8; ++ni) {
        const int lcol = wc * 128 + ni * 16 + ccol;
        for (int r = 0; r < 4; ++r) {
          const int lrow = wr * 32 + mi * 16 + crow_base + r;
          float v = acc[mi][ni][r] + bias[lcol];
          Yimg[lrow][lcol] = f2bf(fast_tanh(v));
        }
      }
    __syncthreads();
  }

  // ---- head: [64, head_dim] = h2 @ W3 + b3 via one MFMA column tile ----
  {
    // wave w handles rows w*16..w*16+15 (16x16 MFMA, cols 0..15)
    f32x4 hacc = {};
    const int hrow = wave * 16 + row_a;
    for (int kt = 0; kt < H / BK; ++kt) {
      bf16x8 af, bf;
      af = *reinterpret_cast<const bf16x8*>(
          &Himg[1][hrow][kt * BK + kseg * 8]);
      for (int i = 0; i < 8; ++i) {
        const int k = kt * BK + kseg * 8 + i;
        bf[i] = (row_a <= n_actions) ? W3t[(int64_t)row_a * H + k] : (__bf16)0.f;
      }
      hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, hacc, 0, 0, 0);
    }
    for (int r = 0; r < 4; ++r) {
      const int lrow = wave * 16 + crow_base + r;
      if (ccol <= n_actions)
        Head[lrow][ccol] = hacc[r] + b3[ccol];
    }
  }
  __syncthreads();

  // ---- categorical sample (== sample_head_kernel math) ----------------
  if (tid < BM) {
    const int gr = bm + tid;
    if (gr < N) {
      const float* row = Head[tid];
      float mx = row[0];
      for (int j = 1; j < n_actions; ++j) mx = fmaxf(mx, row[j]);
      float z = 0.f;
      for (int j = 0; j < n_actions; ++j) z += fast_exp(row[j] - mx);
      const float logz = fast_log(z) + mx;
      uint64_t st = step;
      if (step_base) st += *step_base;
      int a = 0;
      if (greedy) {
        float best = row[0];
        for (int j = 1; j < n_actions; ++j)
          if (row[j] > best) { best = row[j]; a = j; }
      } else {
        const int64_t mg = gr + row_offset;
        const uint64_t r =
            splitmix64(seed ^ (st * 0x51E1F5ull + (uint64_t)mg * 0x9E37ull));
        float u = (float)((r >> 11) * (1.0 / 9007199254740992.0));
        u = fminf(u, 0.999999f);
        float c = 0.f;
        a = n_actions - 1;
        for (int j = 0; j < n_actions; ++j) {
          c += fast_exp(row[j] - logz);
          if (u < c) { a = j; break; }
        }
      }
      actions[gr] = a;
      logp[gr] = row[a] - logz;
      if (value) value[gr] = row[n_actions];
    }
  }
}

// ---------------------------------------------------------------------------
// Device counters (hipGraph support): tiny kernels that advance the RNG /
// optimizer-step counters inside a captured graph, so one captured update
// replays with fresh randomness and correct Adam bias correction.
// ---------------------------------------------------------------------------
__global__ void increment_u64_kernel(unsigned long long* __restrict__ ctr,
                                     unsigned long long delta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *ctr += delta;
}

__global__ void increment_i32_kernel(int* __restrict__ ctr, int delta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *ctr += delta;
}

// ---------------------------------------------------------------------------
// Minibatch shuffle + gather, fused.
//
// The epoch permutation is a 4-round balanced Feistel network over the
// smallest even-bit power-of-two domain >= n, cycle-walked back into [0, n):
// a stateless bijection keyed by (seed, rollout counter, epoch).  This
// replaces host randperm + five giant index-gathers (and is exactly
// reproducible on the CPU oracle: ops/api.feistel_perm).
// ---------------------------------------------------------------------------
// (feistel helpers moved above gemm_kernel: the gather+first-GEMM
// fusion indexes A rows through the permutation)

// One wavefront copies one minibatch row. grid.x = ceil(M/4), block = 256.
// mb_ctr (device) = epoch * minibatches + mb, advanced by increment after
// the gather inside the captured graph; step_base keys the epoch permutation
// to the rollout counter so every update reshuffles.
// TICKET: this launch also advances mb_ctr (no increment kernel follows) —
// see ticket_draw.  TICKET = false is the kernel as it always was: the
// counter stays on the scalar path and so does the whole key schedule.
template <bool TICKET>
__global__ __launch_bounds__(256) void mb_gather_kernel(
    const __bf16* __restrict__ obs_src, const int64_t* __restrict__ act_src,
    const float* __restrict__ logp_src, const float* __restrict__ adv_src,
    const float* __restrict__ ret_src, __bf16* __restrict__ obs_mb,
    int64_t* __restrict__ act_mb, float* __restrict__ logp_mb,
    float* __restrict__ adv_mb, float* __restrict__ ret_mb, int M, int D,
    uint32_t n, int half, uint64_t seed, int minibatches,
    const unsigned long long* __restrict__ step_base,
    unsigned long long* mb_ctr, int skip_obs, unsigned int* ticket) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  unsigned long long ctr;
  if (TICKET) {
    ctr = *(volatile const unsigned long long*)mb_ctr;
    __syncthreads();
    if (threadIdx.x == 0)
      ticket_commit(ticket_draw(ticket), mb_ctr, ctr, 1ull, ticket);
    if (row >= M) return;
  } else {
    if (row >= M) return;
    ctr = *mb_ctr;
  }
  const uint32_t epoch = (uint32_t)(ctr / (unsigned)minibatches);
  const uint32_t mb = (uint32_t)(ctr % (unsigned)minibatches);
  const uint64_t key = splitmix64(seed ^ (*step_base * 0x9E3779B97F4A7C15ull) ^
                                  ((uint64_t)epoch << 32));
  const uint32_t dst = mb * (uint32_t)M + (uint32_t)row;
  const uint32_t src = feistel_perm_idx(dst, n, half, key);

  const __bf16* src_row = obs_src + (int64_t)src * D;
  __bf16* dst_row = obs_mb + (int64_t)row * D;
  if (skip_obs) {
    // gather+first-GEMM fusion: the L1 GEMM / W1 wgrad read obs rows
    // through the permutation themselves — only the small fields copy
  } else if ((D & 3) == 0) {
    // 8-byte chunks (bf16 x4)
    const int chunks = D >> 2;
    const uint64_t* s64 = reinterpret_cast<const uint64_t*>(src_row);
    uint64_t* d64 = reinterpret_cast<uint64_t*>(dst_row);
    for (int c = lane; c < chunks; c += 64) d64[c] = s64[c];
  } else {
    for (int c = lane; c < D; c += 64) dst_row[c] = src_row[c];
  }
  if (lane == 0) {
    act_mb[row] = act_src[src];
    logp_mb[row] = logp_src[src];
    adv_mb[row] = adv_src[src];
    ret_mb[row] = ret_src[src];
  }
}

// ---------------------------------------------------------------------------
// Sequence minibatch gather for recurrent PPO (chunked BPTT): sequences are
// (chunk, env) pairs; sequence s of this minibatch maps through the Feistel
// permutation to a source sequence, and all L of its timesteps are gathered
// so the minibatch tensors are [L, Mseq, ...] (time-major for the BPTT
// loop).  h0/c0 are the saved chunk-boundary recurrent states.
// ---------------------------------------------------------------------------
template <bool TICKET>
__global__ __launch_bounds__(256) void mb_gather_seq_kernel(
    const __bf16* __restrict__ obs_src,   // [T, N, D] flat
    const int64_t* __restrict__ act_src,  // [T, N]
    const float* __restrict__ logp_src, const float* __restrict__ adv_src,
    const float* __restrict__ ret_src,
    const bool* __restrict__ done_src,    // [T, N]
    const float* __restrict__ h0_src,     // [n_chunks, N, H] f32
    const float* __restrict__ c0_src,     // [n_chunks, N, H]
    __bf16* __restrict__ obs_mb,          // [L, Mseq, D]
    int64_t* __restrict__ act_mb,         // [L, Mseq]
    float* __restrict__ logp_mb, float* __restrict__ adv_mb,
    float* __restrict__ ret_mb,
    bool* __restrict__ done_mb,           // [L, Mseq]
    __bf16* __restrict__ h0_mb,           // [Mseq, H] bf16 (GEMM operand)
    float* __restrict__ c0_mb,            // [Mseq, H]
    int Mseq, int L, int D, int H, int N, uint32_t n_seq, int half,
    uint64_t seed, int minibatches,
    const unsigned long long* __restrict__ step_base,
    unsigned long long* mb_ctr, unsigned int* ticket) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);  // seq within mb
  const int lane = threadIdx.x & 63;
  unsigned long long ctr;
  if (TICKET) {
    ctr = *(volatile const unsigned long long*)mb_ctr;
    __syncthreads();
    if (threadIdx.x == 0)
      ticket_commit(ticket_draw(ticket), mb_ctr, ctr, 1ull, ticket);
    if (row >= Mseq) return;
  } else {
    if (row >= Mseq) return;
    ctr = *mb_ctr;
  }
  const uint32_t epoch = (uint32_t)(ctr / (unsigned)minibatches);
  const uint32_t mb = (uint32_t)(ctr % (unsigned)minibatches);
  const uint64_t key = splitmix64(seed ^ (*step_base * 0x9E3779B97F4A7C15ull) ^
                                  ((uint64_t)epoch << 32));
  const uint32_t dst = mb * (uint32_t)Mseq + (uint32_t)row;
  const uint32_t src = feistel_perm_idx(dst, n_seq, half, key);
  const int chunk = (int)(src / (uint32_t)N);
  const int env = (int)(src % (uint32_t)N);
  // recurrent initial state
  {
    const float* hs = h0_src + ((int64_t)chunk * N + env) * H;
    const float* cs = c0_src + ((int64_t)chunk * N + env) * H;
    __bf16* hd = h0_mb + (int64_t)row * H;
    float* cd = c0_mb + (int64_t)row * H;
    for (int j = lane; j < H; j += 64) {
      hd[j] = f2bf(hs[j]);
      cd[j] = cs[j];
    }
  }
  for (int l = 0; l < L; ++l) {
    const int64_t t = (int64_t)chunk * L + l;
    const __bf16* srow = obs_src + (t * N + env) * D;
    __bf16* drow = obs_mb + ((int64_t)l * Mseq + row) * D;
    if ((D & 3) == 0) {
      const int chunks8 = D >> 2;
      const uint64_t* s64 = reinterpret_cast<const uint64_t*>(srow);
      uint64_t* d64 = reinterpret_cast<uint64_t*>(drow);
      for (int c = lane; c < chunks8; c += 64) d64[c] = s64[c];
    } else {
      for (int c = lane; c < D; c += 64) drow[c] = srow[c];
    }
    if (lane == 0) {
      const int64_t si = t * N + env;
      const int64_t di = (int64_t)l * Mseq + row;
      act_mb[di] = act_src[si];
      logp_mb[di] = logp_src[si];
      adv_mb[di] = adv_src[si];
      ret_mb[di] = ret_src[si];
      done_mb[di] = done_src[si];
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

void launch_lstm_cell_fwd(const void* gates_pre, const void* gates_h,
                          const float* c_prev, float* c_new, void* h_new,
                          const bool* done, void* h_masked, float* c_masked,
                          void* acts_out, int64_t M, int H,
                          hipStream_t stream) {
  int64_t total = M * H;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(gates_pre),
                     reinterpret_cast<const __bf16*>(gates_h),
                     c_prev, c_new, reinterpret_cast<__bf16*>(h_new), done,
                     reinterpret_cast<__bf16*>(h_masked), c_masked,
                     reinterpret_cast<__bf16*>(acts_out), M, H);
}

void launch_lstm_cell_bwd(const void* acts, const float* c_prev,
                          const float* c_new, const void* dh_head,
                          const float* dh_next, const float* dc_next,
                          const bool* done, void* dgates, float* dc_prev,
                          int64_t M, int H, hipStream_t stream) {
  int64_t total = M * (H / 4);
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(acts),
                     c_prev, c_new, reinterpret_cast<const __bf16*>(dh_head),
                     dh_next, dc_next, done,
                     reinterpret_cast<__bf16*>(dgates), dc_prev, M, H);
}

bool launch_lstm_gemm_cell_fwd(const void* A, const void* B,
                               const void* gates_pre, void* acts_out,
                               const float* c_prev, float* c_new, void* h_new,
                               const bool* done, void* h_masked,
                               float* c_masked, int M, int N, int K,
                               hipStream_t stream) {
  if (N % 64 != 0) return false;  // 64-col tiles must hold whole units
  dim3 grid(ceil_div(M, 64), N / 64);
  if (acts_out) {
    hipLaunchKernelGGL((lstm_gemm_cell_fwd_kernel<true>), grid, dim3(256), 0,
                       stream, reinterpret_cast<const __bf16*>(A),
                       reinterpret_cast<const __bf16*>(B),
                       reinterpret_cast<const __bf16*>(gates_pre),
                       reinterpret_cast<__bf16*>(acts_out), c_prev, c_new,
                       reinterpret_cast<__bf16*>(h_new), done,
                       reinterpret_cast<__bf16*>(h_masked), c_masked, M, N, K);
  } else {
    hipLaunchKernelGGL((lstm_gemm_cell_fwd_kernel<false>), grid, dim3(256), 0,
                       stream, reinterpret_cast<const __bf16*>(A),
                       reinterpret_cast<const __bf16*>(B),
                       reinterpret_cast<const __bf16*>(gates_pre), nullptr,
                       c_prev, c_new, reinterpret_cast<__bf16*>(h_new), done,
                       reinterpret_cast<__bf16*>(h_masked), c_masked, M, N, K);
  }
  return true;
}

bool launch_lstm_bwd_fused(const void* acts, const float* c_prev,
                           const float* c_new, const void* dh_head,
                           const float* dh_next, const float* dc_next,
                           const bool* done, const void* B, void* dgates,
                           float* dc_prev, float* dh_prev, int M, int H,
                           hipStream_t stream) {
  if (H % 64 != 0) return false;
  dim3 grid(ceil_div(M, 64), dh_prev ? H / 64 : 1);
  hipLaunchKernelGGL(lstm_bwd_fused_kernel, grid, dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(acts), c_prev, c_new,
                     reinterpret_cast<const __bf16*>(dh_head), dh_next,
                     dc_next, done,
                     reinterpret_cast<const __bf16*>(B),
                     reinterpret_cast<__bf16*>(dgates), dc_prev, dh_prev, M,
                     H);
  return true;
}

void launch_mask_reset(void* h, float* c, const bool* done, int64_t M, int H,
                       hipStream_t stream) {
  int64_t total = M * H;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(mask_reset_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<__bf16*>(h), c, done, M, H);
}

void launch_masked_state(const void* h_raw, const float* c_raw,
                         const bool* done, void* h_in, float* c_in, int64_t M,
                         int H, hipStream_t stream) {
  int64_t total = M * H;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(masked_state_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(h_raw), c_raw, done,
                     reinterpret_cast<__bf16*>(h_in), c_in, M, H);
}

void launch_mb_gather_seq(const void* obs_src, const int64_t* act_src,
                          const float* logp_src, const float* adv_src,
                          const float* ret_src, const bool* done_src,
                          const float* h0_src,
                          const float* c0_src, void* obs_mb, int64_t* act_mb,
                          float* logp_mb, float* adv_mb, float* ret_mb,
                          bool* done_mb,
                          void* h0_mb, float* c0_mb, int Mseq, int L, int D,
                          int H, int N, uint32_t n_seq, int half,
                          uint64_t seed, int minibatches,
                          const unsigned long long* step_base,
                          unsigned long long* mb_ctr, unsigned int* ticket,
                          hipStream_t stream) {
#define GATHER_SEQ(TK)                                                        \
  hipLaunchKernelGGL(mb_gather_seq_kernel<TK>, dim3(ceil_div(Mseq, 4)),       \
                     dim3(256), 0, stream,                                    \
                     reinterpret_cast<const __bf16*>(obs_src), act_src,       \
                     logp_src, adv_src, ret_src, done_src, h0_src, c0_src,    \
                     reinterpret_cast<__bf16*>(obs_mb), act_mb, logp_mb,      \
                     adv_mb, ret_mb, done_mb,                                 \
                     reinterpret_cast<__bf16*>(h0_mb), c0_mb, Mseq, L, D, H,  \
                     N, n_seq, half, seed, minibatches, step_base, mb_ctr,    \
                     ticket)
  if (ticket) GATHER_SEQ(true);
  else GATHER_SEQ(false);
#undef GATHER_SEQ
}

void launch_mlp_policy_rollout(const void* obs, const void* W1t,
                               const float* b1, const void* W2t,
                               const float* b2, const void* W3t,
                               const float* b3, int64_t* actions, float* logp,
                               float* value, int N, int D, int n_actions,
                               uint64_t seed, uint64_t step,
                               const unsigned long long* step_base,
                               int row_offset, int greedy,
                               hipStream_t stream) {
  hipLaunchKernelGGL(mlp_policy_rollout_kernel, dim3(ceil_div(N, 64)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(obs),
                     reinterpret_cast<const __bf16*>(W1t), b1,
                     reinterpret_cast<const __bf16*>(W2t), b2,
                     reinterpret_cast<const __bf16*>(W3t), b3, actions, logp,
                     value, N, D, n_actions, seed, step, step_base, row_offset,
                     greedy);
}

void launch_increment_u64(unsigned long long* ctr, unsigned long long delta,
                          hipStream_t stream) {
  hipLaunchKernelGGL(increment_u64_kernel, dim3(1), dim3(1), 0, stream, ctr,
                     delta);
}

void launch_increment_i32(int* ctr, int delta, hipStream_t stream) {
  hipLaunchKernelGGL(increment_i32_kernel, dim3(1), dim3(1), 0, stream, ctr,
                     delta);
}

void launch_mb_gather(const void* obs_src, const int64_t* act_src,
                      const float* logp_src, const float* adv_src,
                      const float* ret_src, void* obs_mb, int64_t* act_mb,
                      float* logp_mb, float* adv_mb, float* ret_mb, int M,
                      int D, uint32_t n, int half, uint64_t seed,
                      int minibatches, const unsigned long long* step_base,
                      unsigned long long* mb_ctr, hipStream_t stream,
                      int skip_obs, unsigned int* ticket) {
#define GATHER(TK)                                                            \
  hipLaunchKernelGGL(mb_gather_kernel<TK>, dim3(ceil_div(M, 4)), dim3(256),   \
                     0, stream, reinterpret_cast<const __bf16*>(obs_src),     \
                     act_src, logp_src, adv_src, ret_src,                     \
                     reinterpret_cast<__bf16*>(obs_mb), act_mb, logp_mb,      \
                     adv_mb, ret_mb, M, D, n, half, seed, minibatches,        \
                     step_base, mb_ctr, skip_obs, ticket)
  if (ticket) GATHER(true);
  else GATHER(false);
#undef GATHER
}

void launch_gemm(const void* A, const void* B, const float* bias, void* C,
                 const void* Yact, int M, int N, int K, bool trans_b, int act,
                 bool dact_tanh, bool add_bias, bool accum,
                 hipStream_t stream, const FeistelMap* fmp = nullptr) {
  const __bf16* a = reinterpret_cast<const __bf16*>(A);
  const __bf16* b = reinterpret_cast<const __bf16*>(B);
  const __bf16* y = reinterpret_cast<const __bf16*>(Yact);
  // tile choice and grid: select_gemm (mfma_dispatch.h), with the knobs
  // this process read from its environment
  const GemmSel s = select_gemm(M, N, K, trans_b, act, dact_tanh, add_bias,
                                accum, fmp != nullptr, process_gemm_knobs());
  const dim3 grid(s.gx, s.gy), block(256);
  const FeistelMap fm = fmp ? *fmp : FeistelMap{};
#define GYMFX_X(TB, ACT, DT, AB, NF, ACC, BK, PERM)                           \
  if (gemm_sel_is(s, TB, ACT, DT, AB, NF, ACC, BK, PERM)) {                   \
    hipLaunchKernelGGL((gemm_kernel<TB, ACT, DT, AB, NF, ACC, BK, PERM>),     \
                       grid, block, 0, stream, a, b, bias, C, y, M, N, K,     \
                       fm);                                                   \
    return;                                                                   \
  }
  GYMFX_GEMM_VARIANTS(GYMFX_X)
#undef GYMFX_X
  // no kernel for this flag combination (a_perm with anything but the L1
  // forward epilogue): unreachable by construction, abort loudly if it
  // ever is
  abort();
}

// Weight-resident tall GEMM (gemm_resident_kernel).  The caller has checked
// gemm_resident_ok; act/dact_tanh pick the epilogue.  max_blocks caps the
// grid (0 = one workgroup per CU, at most one per 256-row group).
void launch_gemm_resident(const void* A, const void* Wt, const float* bias,
                          void* C, const void* Yact, int M, int K, int act,
                          bool dact_tanh, int max_blocks, hipStream_t stream) {
  if (!gemm_resident_ok(M, RESIDENT_N, K, true, act, dact_tanh,
                        bias != nullptr, false))
    abort();
  static const int n_cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess)
      return 256;
    return n;
  }();
  const dim3 grid(gemm_resident_grid(M, n_cus, max_blocks)), block(512);
  const __bf16* a = reinterpret_cast<const __bf16*>(A);
  const __bf16* w = reinterpret_cast<const __bf16*>(Wt);
  const __bf16* y = reinterpret_cast<const __bf16*>(Yact);
  __bf16* c = reinterpret_cast<__bf16*>(C);
#define RESIDENT(EPI, NF, TAIL)                                               \
  hipLaunchKernelGGL((gemm_resident_kernel<EPI, NF, TAIL>), grid, block, 0,   \
                     stream, a, w, bias, c, y, M, K)
#define RESIDENT_EPI(EPI)                                                     \
  do {                                                                        \
    if (K == 256) RESIDENT(EPI, 8, false);                                    \
    else if (K > 256) RESIDENT(EPI, 8, true);                                 \
    else RESIDENT(EPI, -1, false);                                            \
  } while (0)
  // K = 256..264 (the workload's layers) have 8 full chunks: unrolled kernel
  if (dact_tanh) RESIDENT_EPI(1);
  else RESIDENT_EPI(0);
#undef RESIDENT_EPI
#undef RESIDENT
}

void launch_slab_reduce(const float* dW_part, const float* db_part, float* dW,
                        float* db, int N, int K, int slabs, hipStream_t stream);

void launch_wgrad(const void* X, const void* dY, float* dW_part, float* db_part,
                  float* dW, float* db, int M, int N, int K, int slabs,
                  hipStream_t stream, const FeistelMap* fmp = nullptr,
                  bool reduce = true) {
  const __bf16* x = reinterpret_cast<const __bf16*>(X);
  const __bf16* dy = reinterpret_cast<const __bf16*>(dY);
  // tile choice and grid: select_wgrad (mfma_dispatch.h)
  const WgradSel s = select_wgrad(M, N, K, slabs, db_part != nullptr,
                                  fmp != nullptr, process_wgrad_big_knob());
  const dim3 grid(s.gx, s.gy, s.gz);
  const FeistelMap fm = fmp ? *fmp : FeistelMap{};
  bool launched = false;
#define GYMFX_X(DB, FK, FN, PERM)                                             \
  if (wgrad_sel_is(s, true, DB, FK, FN, PERM)) {                              \
    hipLaunchKernelGGL((wgrad_glds_kernel<DB, FK, FN, PERM>), grid,           \
                       dim3(256), 0, stream, x, dy, dW_part, db_part, M, N,   \
                       K, slabs, fm);                                         \
    launched = true;                                                          \
  }
  GYMFX_WGRAD_GLDS_VARIANTS(GYMFX_X)
#undef GYMFX_X
#define GYMFX_X(DB, FK, FN, PERM)                                             \
  if (wgrad_sel_is(s, false, DB, FK, FN, PERM)) {                             \
    hipLaunchKernelGGL((wgrad_partial_kernel<DB, FK, FN, PERM>), grid,        \
                       dim3(256), 0, stream, x, dy, dW_part, db_part, M, N,   \
                       K, slabs, 0, fm);                                      \
    launched = true;                                                          \
  }
  GYMFX_WGRAD_PARTIAL_VARIANTS(GYMFX_X)
#undef GYMFX_X
  if (!launched) abort();  // select_wgrad returned a tile with no kernel
  // reduce == false: the partials stay in dW_part/db_part and
  // launch_grads_finalize reduces every layer's workspace in one launch
  if (!reduce) return;
  launch_slab_reduce(dW_part, db_part, dW, db, N, K, slabs, stream);
}

// The reduce half of launch_wgrad on its own: slab partials -> dW/db (also
// run on the partials head_loss_bwd_kernel wrote when the fused optimizer
// tail is off).
void launch_slab_reduce(const float* dW_part, const float* db_part, float* dW,
                        float* db, int N, int K, int slabs,
                        hipStream_t stream) {
  int64_t elems = (int64_t)K * N;
  if (elems <= 4096) {
    hipLaunchKernelGGL(slab_reduce_small_kernel, dim3((int)elems), dim3(256),
                       0, stream, dW_part, dW, elems, slabs);
  } else {
    int blocks = (int)std::min<int64_t>((elems + 1023) / 1024, 1024);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(256), 0, stream,
                       dW_part, dW, elems, slabs);
  }
  if (db_part && db)
    hipLaunchKernelGGL(slab_reduce_small_kernel, dim3(N), dim3(256), 0, stream,
                       db_part, db, (int64_t)N, slabs);
}

void launch_gae(const float* rewards, const float* values, const bool* dones,
                float* adv, float* ret, int T, int N, float gamma, float lam,
                hipStream_t stream) {
  hipLaunchKernelGGL(gae_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream,
                     rewards, values, dones, adv, ret, T, N, gamma, lam);
}

void launch_adam(float* p, const float* g, float* m, float* v, void* p_bf16,
                 int64_t n, float lr, float beta1, float beta2, float eps,
                 float bc1, float bc2, const float* gscale, const int* step_ctr,
                 hipStream_t stream) {
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, stream, p, g, m,
                     v, reinterpret_cast<__bf16*>(p_bf16), n, lr, beta1, beta2,
                     eps, bc1, bc2, gscale, step_ctr, nullptr, 0, 0.f);
}

void launch_adam_clip(float* p, const float* g, float* m, float* v,
                      void* p_bf16, int64_t n, float lr, float beta1,
                      float beta2, float eps, float bc1, float bc2,
                      const int* step_ctr, const float* clip_part, int nparts,
                      float max_norm, hipStream_t stream) {
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, stream, p, g, m,
                     v, reinterpret_cast<__bf16*>(p_bf16), n, lr, beta1, beta2,
                     eps, bc1, bc2, nullptr, step_ctr, clip_part, nparts,
                     max_norm);
}

void launch_grad_clip(const float* g, int64_t n, float max_norm, float* part,
                      float* scale, int nparts, hipStream_t stream) {
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nparts), dim3(256), 0, stream,
                     g, n, part);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, stream, part,
                     nparts, max_norm, scale);
}

void launch_grad_sumsq(const float* g, int64_t n, float* part, int nparts,
                       hipStream_t stream) {
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nparts), dim3(256), 0, stream,
                     g, n, part);
}

void launch_grads_finalize(const FinalizeTable& tab, float* grads, int64_t n,
                           float* clip_part, hipStream_t stream) {
  // with norm partials the grid IS the 256-partial layout of
  // sumsq_partial_kernel; without, no more blocks than there is work
  const int blocks =
      clip_part ? 256 : (int)std::min<int64_t>((n + 255) / 256, 256);
  hipLaunchKernelGGL(grads_finalize_kernel, dim3(blocks), dim3(1024), 0,
                     stream, tab, grads, n, clip_part);
}

void launch_adam_tail(float* p, const float* g, float* m, float* v,
                      void* p_bf16, int64_t n, float lr, float beta1,
                      float beta2, float eps, int* step_ctr,
                      unsigned int* ticket, const float* clip_part, int nparts,
                      float max_norm, const MirrorTable& mt,
                      hipStream_t stream) {
  int blocks = (int)std::min<int64_t>((n + 1023) / 1024, 2048);
  hipLaunchKernelGGL(adam_tail_kernel, dim3(blocks), dim3(1024), 0, stream, p,
                     g, m, v, reinterpret_cast<__bf16*>(p_bf16), n, lr, beta1,
                     beta2, eps, step_ctr, ticket, clip_part, nparts, max_norm,
                     mt);
}

void launch_sample_head(const float* head, int M, int n_actions, uint64_t seed,
                        uint64_t step, int64_t* actions, float* logp,
                        float* value, float* entropy, int greedy,
                        const unsigned long long* step_base, int row_offset,
                        hipStream_t stream) {
  hipLaunchKernelGGL(sample_head_kernel, dim3(ceil_div(M, 256)), dim3(256), 0,
                     stream, head, M, n_actions, seed, step, actions, logp,
                     value, entropy, greedy, step_base, row_offset);
}

void launch_ppo_loss_bwd(const float* head, const int64_t* actions,
                         const float* old_logp, const float* adv,
                         const float* ret, void* dhead, int M, int n_actions,
                         float clip_eps, float ent_coef, float vf_coef,
                         float inv_count, float* losses, hipStream_t stream) {
  hipLaunchKernelGGL(ppo_loss_bwd_kernel, dim3(ceil_div(M, 256)), dim3(256), 0,
                     stream, head, actions, old_logp, adv, ret,
                     reinterpret_cast<__bf16*>(dhead), M, n_actions, clip_eps,
                     ent_coef, vf_coef, inv_count, losses);
}

// hidden == 256, head_dim <= 16 and ceil(M/slabs) <= 128 are the caller's
// to check (bindings.cpp: head_loss_bwd_op)
void launch_head_loss_bwd(const void* h2, const void* W3t, const void* W3,
                          const float* b3, const int64_t* actions,
                          const float* old_logp, const float* adv,
                          const float* ret, float* head, void* dhead,
                          void* dh2, float* dW_part, float* db_part, int M,
                          int head_dim, int slabs, float clip_eps,
                          float ent_coef, float vf_coef, float inv_count,
                          float* losses, int loss_shards, hipStream_t stream) {
  hipLaunchKernelGGL(head_loss_bwd_kernel, dim3(slabs), dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(h2),
                     reinterpret_cast<const __bf16*>(W3t),
                     reinterpret_cast<const __bf16*>(W3), b3, actions,
                     old_logp, adv, ret, head,
                     reinterpret_cast<__bf16*>(dhead),
                     reinterpret_cast<__bf16*>(dh2), dW_part, db_part, M,
                     head_dim, slabs, clip_eps, ent_coef, vf_coef, inv_count,
                     losses, loss_shards);
}

void launch_adv_normalize(float* adv, int64_t n, float* part, int nparts,
                          hipStream_t stream) {
  hipLaunchKernelGGL(adv_norm_stats_kernel, dim3(nparts), dim3(256), 0, stream,
                     adv, n, part);
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adv_norm_apply_kernel, dim3(blocks), dim3(256), 0, stream,
                     adv, n, part, nparts);
}

void launch_transpose_bf16(const void* src, void* dst, int K, int N,
                           hipStream_t stream) {
  dim3 grid(ceil_div(K, 64), ceil_div(N, 64));
  hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(src),
                     reinterpret_cast<__bf16*>(dst), K, N);
}

void launch_f32_to_bf16(const float* in, void* out, int64_t n,
                        hipStream_t stream) {
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(blocks), dim3(256), 0, stream, in,
                     reinterpret_cast<__bf16*>(out), n);
}

}  // namespace gymfx
