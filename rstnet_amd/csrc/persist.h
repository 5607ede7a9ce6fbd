// In-launch all-to-all hand-offs of the persistent frame kernels (lm_depth.hip, lm_temporal.hip, codec_tr.hip) and, below the device
// helpers, the host half of their launches: residency probe and launch pair.  An op's output vector lives in a
// global array of 8-byte {epoch tag, fp32 value} granules, each written by ONE relaxed agent-scope (sc1, write-through) store;
// a consuming workgroup sweeps the granules it needs with relaxed agent-scope loads until every tag equals the op's epoch and
// stages the values in LDS (cdna_hip_programming.md Guideline 16, form R2: the data is the flag -- no fence, no dispatch-order or
// placement assumption).  The workspace is zeroed by a memset node in front of every launch (epochs count from 1 inside a
// launch); every spin is bounded: a timeout sets the workgroup's `dead` flag (later waits do not spin again) and ORs a code into
// the caller's status word, so the launch always terminates.
//
// Safety net (round 3): the launches need every workgroup resident at once, which a shared device does not promise.  Each launcher
// (1) sizes the grid so that EVERY workgroup publishes in the all-to-all ops that separate two writes of a buffer (a workgroup that
// owned no rows there could lag and find its buffer overwritten), (2) refuses shapes the occupancy query says cannot be resident,
// and (3) enqueues, right behind the persistent launch, the SAME kernel as ONE workgroup (`SOLO`): it returns at once when
// status[0] == 0 and otherwise recomputes the whole frame alone -- a single workgroup depends on nobody, so it cannot time out --
// overwriting the outputs, then bumps status[1] (frames repaired), ORs the codes into status[2] and clears status[0].  Wrong
// outputs therefore never leave the stream; the host reads status[1] now and then and retires the persistent path for a device
// that keeps failing (a repaired frame costs the time-outs plus ~30 ms).
#pragma once
#include <type_traits>

#include "lm_common.h"

namespace {

constexpr int DF_THREADS = 256, DF_WAVES = 4;
constexpr long long DF_TIMEOUT_TICKS = 10000000;   // of the 100 MHz wall clock (s_memrealtime): a lost hand-off costs 0.1 s, once per workgroup
constexpr int DF_HDR_FLOATS = 512;     // DfShared in the first KB of the header, the sampler's scratch in the second
typedef unsigned long long u64;
#define DF_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void df_publish(u64* g, unsigned epoch, float v) {
    __hip_atomic_store(g, ((u64)epoch << 32) | (u64)__float_as_uint(v), DF_RLX);
}

struct DfShared {
    float red[DF_WAVES];
    long tok[2];
    float tokf[2];
    int dead;              // a wait of this workgroup timed out: later waits do not spin again
    int pad;
};

// Sweep `n` granules (source index of item i = map(i)) until every tag == epoch; values -> dst[i] (LDS).  All threads of the
// workgroup take part (up to GP granules per thread and pass, all requested before any is examined).  ONE sweep in flight per
// workgroup, re-issued when it returns: both variations measured in round 4 were slower (profiles/r04_handoff_polling.txt) -- a
// second sweep in flight (half the detection delay on paper) doubles 2-6 TB/s of fabric traffic that the publishing stores and the
// next op's weight prefetch queue behind (+1 to +4 us per hand-off); watching one sentinel granule per thread first and sweeping
// when it turns adds a round trip (+0.3 to +0.7 us per hand-off).
template <int GP, typename Map>
__device__ __forceinline__ void df_gather(const u64* g, int n, unsigned epoch, float* dst, Map map, DfShared& sh, unsigned* status, unsigned code) {
    const int tid = threadIdx.x;
    __syncthreads();        // dst may still be read by the rows of the previous op (another wave of this workgroup)
    for (int base = 0; base < n; base += GP * DF_THREADS) {
        u64 v[GP];
        long long t0 = 0;
        while (true) {
            bool all = true;
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                const int i = base + j * DF_THREADS + tid;
                v[j] = i < n ? __hip_atomic_load(g + map(i), DF_RLX) : ((u64)epoch << 32);
            }
#pragma unroll
            for (int j = 0; j < GP; ++j) all = all && (unsigned)(v[j] >> 32) == epoch;
            if (all) break;
            // time-based bound: how long a poll takes depends on what else the chip is doing (a count of polls measured 10x apart)
            if (t0 == 0) t0 = wall_clock64();
            if (*(volatile int*)&sh.dead || wall_clock64() - t0 > DF_TIMEOUT_TICKS) {
                sh.dead = 1;
                atomicOr(status, code);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            const int i = base + j * DF_THREADS + tid;
            if (i < n) dst[i] = __uint_as_float((unsigned)v[j]);
        }
    }
    __syncthreads();
}

// The weight-row worker of lm_depth.hip (bf16 weights, F32W = false) and codec_tr.hip (fp32 weights, F32W = true):
// rows r = gw, gw + W, ... of w [N][K] against xs [B][K] (LDS), in blocks of RU rows x CU chunks of 512 k whose loads are
// all requested before the first is used.  PAIR: "row" q stands for the rows (q, N/2 + q) of a stacked gated layer.
// The FIRST block (rows gw + j W, k < CU * 512 -- the whole op at the depth transformer's real shape) can be requested ahead of
// time: df_rows_issue() before the hand-off that produces xs, df_rows() after it -- the weights do not depend on activations, so
// their HBM latency hides behind the wait (the "prefetch-credit" of MI355X_MICROARCH.md's price list).  epi(row, sums) on lane 0.
// k order: ONE fmaf chain per (row, batch row) and lane, gemv_kernel's (lm_step.hip) -- the lane's 8 k of every 512-wide chunk,
// chunks ascending, through the same WChunk::dot; the 64 lanes then meet in wave_sum_fast (DPP steps where gemv_kernel has the
// wave_sum butterfly: the one difference in arithmetic, the order of the additions across lanes).
template <bool F32W, int RU, int CU, bool PAIR> struct DfPre { WChunk<F32W> wv[RU][PAIR ? 2 : 1][CU]; };
template <bool F32W> using df_weight_t = std::conditional_t<F32W, float, unsigned short>;

template <bool F32W, int RU, int CU, bool PAIR>
__device__ __forceinline__ void df_rows_load(DfPre<F32W, RU, CU, PAIR>& pre, const df_weight_t<F32W>* w, int rows, int K, int r0, int kb, int W, int lane) {
    constexpr int HV = PAIR ? 2 : 1;
#pragma unroll
    for (int j = 0; j < RU; ++j)
#pragma unroll
        for (int h = 0; h < HV; ++h)
#pragma unroll
            for (int c = 0; c < CU; ++c) {
                const int r = r0 + j * W, kk = kb + c * 512 + lane * 8;
                pre.wv[j][h][c].zero();
                if (r < rows && kk < K) pre.wv[j][h][c].load(w, ((long)r + (long)h * rows) * K + kk);
            }
}

template <bool F32W, int RU, int CU, bool PAIR>
__device__ __forceinline__ void df_rows_issue(DfPre<F32W, RU, CU, PAIR>& pre, const df_weight_t<F32W>* w, int N, int K, int gw, int W, int lane) {
    df_rows_load(pre, w, PAIR ? N / 2 : N, K, gw, 0, W, lane);
}

template <int B, bool F32W, int RU, int CU, bool PAIR, typename Epi>
__device__ __forceinline__ void df_rows(DfPre<F32W, RU, CU, PAIR>& pre, const df_weight_t<F32W>* w, int N, int K, const float* xs, int gw, int W, int lane,
                                        Epi epi) {
    constexpr int HV = PAIR ? 2 : 1;
    const int rows = PAIR ? N / 2 : N;
    for (int r0 = gw; r0 < rows; r0 += RU * W) {
        float acc[RU][HV][B];
#pragma unroll
        for (int j = 0; j < RU; ++j)
#pragma unroll
            for (int h = 0; h < HV; ++h)
#pragma unroll
                for (int b = 0; b < B; ++b) acc[j][h][b] = 0.f;
        for (int kb = 0; kb < K; kb += CU * 512) {
            if (r0 != gw || kb != 0) df_rows_load(pre, w, rows, K, r0, kb, W, lane);     // the first block was issued ahead
#pragma unroll
            for (int c = 0; c < CU; ++c) {
                const int kk = kb + c * 512 + lane * 8;
                if (kk < K) {
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        const f32x4 x0 = *reinterpret_cast<const f32x4*>(xs + b * K + kk);
                        const f32x4 x1 = *reinterpret_cast<const f32x4*>(xs + b * K + kk + 4);
#pragma unroll
                        for (int j = 0; j < RU; ++j)
#pragma unroll
                            for (int h = 0; h < HV; ++h) acc[j][h][b] = pre.wv[j][h][c].dot(x0, x1, acc[j][h][b]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RU; ++j) {
            const int r = r0 + j * W;
            float s[HV][B];
#pragma unroll
            for (int h = 0; h < HV; ++h)
#pragma unroll
                for (int b = 0; b < B; ++b) s[h][b] = wave_sum_fast(acc[j][h][b]);
            if (lane == 0 && r < rows) epi(r, s);
        }
    }
}

// End of a SOLO (repair) launch: the frame was recomputed by this one workgroup.
__device__ __forceinline__ void df_solo_done(unsigned* status) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned code = __hip_atomic_load(status, DF_RLX);
        __hip_atomic_fetch_add(status + 1, 1u, DF_RLX);
        __hip_atomic_fetch_or(status + 2, code, DF_RLX);
        __hip_atomic_store(status, 0u, DF_RLX);
    }
}

// ---- host half: the launch contract of the three persistent kernels (lm_depth.hip, lm_temporal.hip, codec_tr.hip) ---------------
// A shape is served when its LDS footprint is within DF_LDS_LIMIT, its grid (at most one workgroup per CU, every workgroup owning rows
// of every all-to-all op) has a workgroup per head, and one workgroup of that footprint fits a CU (df_fits_cu).  A call enqueues
// three stream operations (df_launch_pair): the memset of BOTH granule sets, the grid, the one-workgroup repair launch.
constexpr size_t DF_LDS_LIMIT = 150 * 1024;    // dynamic LDS the kernels opt in to: the gate of every shape, the probe, the launch

// The workspace holds two sets of `n` granules: the persistent launch's, then the repair launch's (the kernels: gran + SOLO * n).
inline size_t df_both_sets_bytes(long n) { return 2 * (size_t)n * sizeof(u64); }

// Largest grid (<= `cus`) in which every workgroup (4 waves, row r -> wave r mod 4G) owns a row of an op with `min_rows` rows.
inline int df_grid_for_rows(int cus, int min_rows) {
    const int g = (min_rows + DF_WAVES - 1) / DF_WAVES;
    return g < cus ? (g < 1 ? 1 : g) : cus;
}

// Residency: all workgroups of a persistent launch must run at once, one per CU -- whether a CU of the current device takes one workgroup
// of KERN with `probe_bytes` of dynamic LDS.  Asked once per (device, kernel instance, footprint class `cls` < CLASSES: the answer does
// not change within a class); a device ordinal the table does not cover is asked every time (rst_device_cell).
template <auto KERN, int CLASSES = 1>
bool df_fits_cu(int threads, size_t probe_bytes, int cls = 0) {
    static signed char fits[RST_MAX_DEVICES][CLASSES];      // 0 = not asked yet, 1 = fits, -1 = does not
    signed char uncached = 0;
    signed char& f = rst_device_cell(&fits[0][cls], CLASSES, uncached);
    if (f == 0) {
        rst_allow_dynamic_lds<KERN>((int)DF_LDS_LIMIT);
        int nb = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, KERN, threads, probe_bytes);
        (void)hipGetLastError();
        f = (e == hipSuccess && nb >= 1) ? 1 : -1;
    }
    return f > 0;
}

// One persistent call: every polled word of both granule sets starts at zero in EVERY launch (a memset node when captured: epochs count
// from 1), then PERSISTENT on `grid` workgroups and, behind it in the stream, SOLO as one workgroup (a no-op unless a hand-off timed out).
template <auto PERSISTENT, auto SOLO, typename P>
int df_launch_pair(const char* what, const P& p, int grid, int threads, size_t lds, u64* gran, long granules, hipStream_t stream, bool repair = true) {
    if (hipMemsetAsync(gran, 0, df_both_sets_bytes(granules), stream) != hipSuccess) {
        rst_set_error("%s: workspace memset failed", what);
        return RST_ERR_LAUNCH;
    }
    rst_allow_dynamic_lds<PERSISTENT>((int)DF_LDS_LIMIT);
    hipLaunchKernelGGL(PERSISTENT, dim3(grid), dim3(threads), lds, stream, p);
    if (repair) {
        rst_allow_dynamic_lds<SOLO>((int)DF_LDS_LIMIT);
        hipLaunchKernelGGL(SOLO, dim3(1), dim3(threads), lds, stream, p);
    }
    return rst_check_launch(what);
}

}  // namespace
