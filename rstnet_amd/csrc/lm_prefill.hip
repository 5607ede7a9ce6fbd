// Multi-position (prefill) attention of the LM temporal transformer: Tc new positions of B streams against the ring PLUS the chunk
// itself, before anything is appended, and the append that follows it in stream order.
//
// A query at position p sees keys j with max(0, p - window + 1) <= j <= p.  Keys at positions < pos (= *pos_dev, the chunk's first
// position) are read from ring slot j % cap; keys at positions >= pos come from the chunk's own qkv rows, rotated and rounded to the
// ring's dtype first, so a query sees exactly the bytes a later step reads back from the ring.  The append is a separate launch
// because slot (pos + t) % cap of new position pos + t is the slot of old position pos + t - cap, which the chunk's first queries
// still need once the ring has wrapped.
//
// Launches of rst_launch_lm_attn_prefill:
//   1. stage_kernel: rotated queries (fp32) and the chunk's rotated keys / values (ring dtype) into the caller's workspace;
//   2. bf16 rings: prefill_attn_bf16_kernel -- v_mfma_f32_32x32x16_bf16 in online-softmax form over 32-key tiles, one workgroup per
//      (32 queries, head, stream), its four waves taking every fourth key tile and merging through LDS;
//      fp32 rings (tiny models, kv_dtype=float32: the parity configuration): prefill_attn_f32_kernel, plain fp32 FMAs.
// rst_launch_lm_ring_append is stage_kernel again with the ring as its destination: the same instructions produce the same bytes.
//
// Grouped KV heads (G < H, the litgpt-style GPT): the qkv row is [q: H*D | k: G*D | v: G*D], rings and the staged keys / values hold
// G heads, and query head h reads KV head h / (H / G).  G == H is the Moshi layout, with the index arithmetic it always had.
#include "lm_common.h"

namespace {

typedef short pf_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pf_f32x2 __attribute__((ext_vector_type(2)));

template <bool KV16> struct PfKv;
template <> struct PfKv<false> {
    typedef float elem;
    static __device__ __forceinline__ void store2(void* base, long at, float a, float b) {
        *reinterpret_cast<pf_f32x2*>(static_cast<float*>(base) + at) = pf_f32x2{a, b};
    }
};
template <> struct PfKv<true> {
    typedef unsigned short elem;
    static __device__ __forceinline__ void store2(void* base, long at, float a, float b) {
        *reinterpret_cast<unsigned*>(static_cast<unsigned short*>(base) + at) = (unsigned)bf16_rne(a) | ((unsigned)bf16_rne(b) << 16);
    }
};

// One (real, imag) pair of one head of one new position per work item (the arithmetic of rope_append_kernel, lm_attn.hip:
// angle = exp(i * rope_coef) * position as an fp32 product, cosf / sinf of it).  to_ring == 0: q heads -> q_rot [B][H][T][D] fp32, k / v heads -> k_new / v_new
// [B][G][T][D] in the ring's dtype.  to_ring != 0: k / v heads only -> ring slots (pos + t) % cap of [B][G][cap][D].
template <bool KV16>
__global__ __launch_bounds__(256) void stage_kernel(const LmPrefillParams p, const int to_ring) {
    const int half = p.D / 2;
    const int nh = to_ring ? p.G : p.H + p.G;
    const long total = (long)p.B * p.T * nh * half;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int i = (int)(idx % half);
        const int hh = (int)((idx / half) % nh) + (to_ring ? p.H : 0);
        const int t = (int)((idx / ((long)half * nh)) % p.T);
        const long b = idx / ((long)half * nh * p.T);
        const long pos = p.pos_dev[b * p.pos_stride] + t;      // (stride 0: every lane reads the one shared word)
        // ragged append: rows at or past the stream's length leave their ring slots as they are (a length <= t0 takes nothing)
        if (to_ring && p.lengths && t >= p.lengths[b] - p.t0) continue;
        const float* row = p.qkv + (b * p.T + t) * (long)p.ldqkv;
        float c = 1.f, s = 0.f;
        if (p.rope && 2 * i < p.rope_dims) {
            // a one-ulp difference in the frequency is multiplied by the position (3000 * 6e-8 = 1.8e-4 rad, measured as 1.9e-4 relative
            // on the stored keys of a chunk at positions 2900 .. 3155 with expf here).  So the caller may hand in the fp32 frequencies its
            // reference uses (rope_freqs); without them: the correctly rounded fp32 value of exp(i * rope_coef)
            const float fr = p.rope_freqs ? p.rope_freqs[i] : (float)exp((double)((float)i * p.rope_coef));
            const float ang = fr * (float)pos;
            c = cosf(ang);
            s = sinf(ang);
        }
        if (hh < p.H) {
            const float qr = row[(long)hh * p.D + 2 * i], qi = row[(long)hh * p.D + 2 * i + 1];
            float* qd = p.q_rot + ((b * p.H + hh) * p.T + t) * (long)p.D + 2 * i;
            *reinterpret_cast<pf_f32x2*>(qd) = pf_f32x2{qr * c - qi * s, qr * s + qi * c};
        } else {
            const int g = hh - p.H;
            const float* ks = row + ((long)p.H + g) * p.D + 2 * i;
            const float* vs = ks + (long)p.G * p.D;
            const long at = to_ring ? ((b * p.G + g) * p.cap + (long)(pos % p.cap)) * p.D + 2 * i
                                    : ((b * p.G + g) * p.T + t) * (long)p.D + 2 * i;
            PfKv<KV16>::store2(to_ring ? p.k : p.k_new, at, ks[0] * c - ks[1] * s, ks[0] * s + ks[1] * c);
            PfKv<KV16>::store2(to_ring ? p.v : p.v_new, at, vs[0], vs[1]);
        }
    }
}

// Positions are handled RELATIVE to pos: query t in [0, T), key u in [-window + 1, T).  u < 0: ring slot (pos % cap + u) mod cap;
// u >= 0: row u of the staged chunk.  Key u is visible to query t iff max(t - window + 1, -pos) <= u <= t.

// ---- fp32 rings: one wave per (query, head, stream); lane = every 64th key, the whole head dim in registers
template <int D>
__global__ __launch_bounds__(64) void prefill_attn_f32_kernel(const LmPrefillParams p) {
    __shared__ __attribute__((aligned(16))) float sm_q[D];
    const int lane = threadIdx.x, t = blockIdx.x, h = blockIdx.y;
    const long b = blockIdx.z;
    const long pos = p.pos_dev[b * p.pos_stride];
    const int pos_mod = (int)(pos % p.cap);
    const int u_min = -(int)min(pos, (long)p.cap);
    const int u_lo = max(t - p.window + 1, u_min);
    const float* qrow = p.q_rot + ((b * p.H + h) * p.T + t) * (long)D;
    for (int i = lane; i < D; i += 64) sm_q[i] = qrow[i];
    __syncthreads();
    const long bg = b * p.G + h / (p.H / p.G);          // this query head's KV head
    const float* kring = static_cast<const float*>(p.k) + bg * (long)p.cap * D;
    const float* vring = static_cast<const float*>(p.v) + bg * (long)p.cap * D;
    const float* knew = static_cast<const float*>(p.k_new) + bg * (long)p.T * D;
    const float* vnew = static_cast<const float*>(p.v_new) + bg * (long)p.T * D;
    const float scale = 1.0f / sqrtf((float)D);
    float m_run = -INFINITY, l_run = 0.f;
    float o[D];
#pragma unroll
    for (int i = 0; i < D; ++i) o[i] = 0.f;
    for (int u = u_lo + lane; u <= t; u += 64) {
        const float *kr, *vr;
        if (u < 0) {
            int s = pos_mod + u;
            if (s < 0) s += p.cap;
            kr = kring + (long)s * D; vr = vring + (long)s * D;
        } else {
            kr = knew + (long)u * D; vr = vnew + (long)u * D;
        }
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < D; i += 4) {
            const f32x4 kk = *reinterpret_cast<const f32x4*>(kr + i);
            const f32x4 qq = *reinterpret_cast<const f32x4*>(sm_q + i);
            d = fmaf(kk[0], qq[0], d); d = fmaf(kk[1], qq[1], d); d = fmaf(kk[2], qq[2], d); d = fmaf(kk[3], qq[3], d);
        }
        const float sc = d * scale;
        const float m_new = fmaxf(m_run, sc);
        const float alpha = m_run == -INFINITY ? 0.f : expf(m_run - m_new);
        const float pw = expf(sc - m_new);
        l_run = l_run * alpha + pw;
#pragma unroll
        for (int i = 0; i < D; i += 4) {
            const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + i);
            o[i] = fmaf(pw, vv[0], o[i] * alpha); o[i + 1] = fmaf(pw, vv[1], o[i + 1] * alpha);
            o[i + 2] = fmaf(pw, vv[2], o[i + 2] * alpha); o[i + 3] = fmaf(pw, vv[3], o[i + 3] * alpha);
        }
        m_run = m_new;
    }
    const float m_w = wave_max(m_run);                 // (the query's own key is always visible: m_w is finite)
    const float f = m_run == -INFINITY ? 0.f : expf(m_run - m_w);
    const float l_w = wave_sum(l_run * f);
    float* out = p.out + ((b * p.T + t) * p.H + h) * (long)D;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float v = wave_sum(o[i] * f);
        if (lane == (i & 63)) out[i] = v / l_w;
    }
}

// ---- bf16 rings: S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16_bf16.
// Operand maps (lane l: r = l & 31, hf = l >> 5): A[row r][k = 8 hf + j], B[k = 8 hf + j][col r], j = 0..7;
// C / D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 hf.
// Scores: A = a 32-key tile (16 contiguous bytes of the key row per lane and k-step: ring keys enter exactly), B = Q^T as bf16 hi + lo
// (two MFMAs per k-step), so the score tile has the QUERY on the lane and the keys in the 16 registers: the softmax statistics of a
// query are 16 registers and one cross-half exchange.  That tile is the B operand of the second product with no data movement:
// registers 8 s .. 8 s + 7 are the fragment of k-step s, whose element j is key 16 s + 8 (j >> 2) + 4 hf + (j & 3) -- the V^T
// fragment (A, row = head dim) gathers the same keys.  Probabilities enter as bf16 hi + lo; accumulation and softmax are fp32.
template <int D>
__global__ __launch_bounds__(256) void prefill_attn_bf16_kernel(const LmPrefillParams p) {
    constexpr int KS = D / 16;     // k-steps of the score product
    constexpr int NT = D / 32;     // 32-dim tiles of the output
    __shared__ __attribute__((aligned(16))) float sm_o[D * 32];    // [head dim][query]
    __shared__ float sm_m[32], sm_l[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, hf = lane >> 5;
    const int t0 = blockIdx.x * 32, h = blockIdx.y;
    const long b = blockIdx.z;
    const long pos = p.pos_dev[b * p.pos_stride];
    const int pos_mod = (int)(pos % p.cap);
    const int u_min = -(int)min(pos, (long)p.cap);
    const int t_last = min(t0 + 31, p.T - 1);
    const int u_lo = max(t0 - p.window + 1, u_min);
    const int n_tiles = (t_last - u_lo) / 32 + 1;
    const int tq = t0 + r;                               // this lane's query; rows past T are computed on a clamped row and dropped
    const int q_lo = max(tq - p.window + 1, u_min);      // its visible keys: q_lo <= u <= tq

    const long bg = b * p.G + h / (p.H / p.G);          // this query head's KV head (workgroup-uniform: scalar registers)
    const unsigned short* kring = static_cast<const unsigned short*>(p.k) + bg * (long)p.cap * D;
    const unsigned short* vring = static_cast<const unsigned short*>(p.v) + bg * (long)p.cap * D;
    const unsigned short* knew = static_cast<const unsigned short*>(p.k_new) + bg * (long)p.T * D;
    const unsigned short* vnew = static_cast<const unsigned short*>(p.v_new) + bg * (long)p.T * D;
    // row (in elements) of key u in its source, and whether that source is the staged chunk; u is clamped into [u_lo, t_last] (a
    // clamped key is masked by its score, its bytes are finite ring / chunk contents)
    auto row_of = [&](int u, bool& is_new) -> long {
        u = min(max(u, u_lo), t_last);
        is_new = u >= 0;
        int s = pos_mod + u;
        if (s < 0) s += p.cap;
        return (long)(is_new ? u : s) * D;
    };

    pf_bf16x8 qh[KS], ql[KS];
    {
        const float* qrow = p.q_rot + ((b * p.H + h) * p.T + min(tq, p.T - 1)) * (long)D;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float v[8];
            const f32x4 a = *reinterpret_cast<const f32x4*>(qrow + 16 * s + 8 * hf);
            const f32x4 c = *reinterpret_cast<const f32x4*>(qrow + 16 * s + 8 * hf + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = c[e]; }
            u32x4 hi, lo;
            split_hi_lo8(v, hi, lo);
            qh[s] = __builtin_bit_cast(pf_bf16x8, hi);
            ql[s] = __builtin_bit_cast(pf_bf16x8, lo);
        }
    }
    const float scale = 1.0f / sqrtf((float)D);
    float m_run = -INFINITY, l_run = 0.f;     // l_run: this lane half's share of the query's sum
    f32x16 o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[n][i] = 0.f;

    for (int tile = wave; tile < n_tiles; tile += 4) {
        const int ub = u_lo + tile * 32;
        f32x16 sc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[i] = 0.f;
        {
            bool is_new;
            const long at = row_of(ub + r, is_new);
            const unsigned short* kr = (is_new ? knew : kring) + at + 8 * hf;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const pf_bf16x8 a = *reinterpret_cast<const pf_bf16x8*>(kr + 16 * s);
                sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qh[s], sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ql[s], sc, 0, 0, 0);
            }
        }
        float m_new = m_run;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int u = ub + (i & 3) + 8 * (i >> 2) + 4 * hf;
            sc[i] = (u >= q_lo && u <= tq) ? sc[i] * scale : -INFINITY;
            m_new = fmaxf(m_new, sc[i]);
        }
        m_new = fmaxf(m_new, __shfl_xor(m_new, 32));
        const float m_ref = m_new == -INFINITY ? 0.f : m_new;      // nothing visible yet: every weight below is exp(-inf) = 0
        const float alpha = m_run == -INFINITY ? 0.f : expf(m_run - m_ref);
        float pw[16];
        float l_add = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            pw[i] = expf(sc[i] - m_ref);
            l_add += pw[i];
        }
        l_run = l_run * alpha + l_add;
        m_run = m_new;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[n][i] *= alpha;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = pw[8 * s + j];
            u32x4 hi, lo;
            split_hi_lo8(v, hi, lo);
            const pf_bf16x8 ph = __builtin_bit_cast(pf_bf16x8, hi), pl = __builtin_bit_cast(pf_bf16x8, lo);
            // the 8 keys of this fragment (the same for every lane of the half): two runs of four
            const unsigned short* vr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bool is_new;
                const long at = row_of(ub + 16 * s + 8 * (j >> 2) + 4 * hf + (j & 3), is_new);
                vr[j] = (is_new ? vnew : vring) + at + r;
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                pf_bf16x8 a;
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = (short)vr[j][32 * n];
                o[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ph, o[n], 0, 0, 0);
                o[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pl, o[n], 0, 0, 0);
            }
        }
    }
    l_run += __shfl_xor(l_run, 32);

    // merge waves 1..3 into wave 0, one at a time through one LDS image
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
            if (hf == 0) { sm_m[r] = m_run; sm_l[r] = l_run; }
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) sm_o[(32 * n + (i & 3) + 8 * (i >> 2) + 4 * hf) * 32 + r] = o[n][i];
        }
        __syncthreads();
        if (wave == 0) {
            const float m_o = sm_m[r], l_o = sm_l[r];
            const float m_new = fmaxf(m_run, m_o);
            const float m_ref = m_new == -INFINITY ? 0.f : m_new;
            const float fa = m_run == -INFINITY ? 0.f : expf(m_run - m_ref);
            const float fb = m_o == -INFINITY ? 0.f : expf(m_o - m_ref);
            l_run = l_run * fa + l_o * fb;
            m_run = m_new;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    o[n][i] = o[n][i] * fa + sm_o[(32 * n + (i & 3) + 8 * (i >> 2) + 4 * hf) * 32 + r] * fb;
        }
        __syncthreads();
    }
    if (wave == 0 && tq < p.T) {
        const float inv = 1.0f / l_run;
        float* out = p.out + ((b * p.T + tq) * p.H + h) * (long)D;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4*>(out + 32 * n + 8 * g + 4 * hf) =
                    f32x4{o[n][4 * g] * inv, o[n][4 * g + 1] * inv, o[n][4 * g + 2] * inv, o[n][4 * g + 3] * inv};
    }
}

int prefill_check(const LmPrefillParams& p, const char* what, bool attention) {
    RST_REQUIRE(p.qkv && p.k && p.v && p.pos_dev && p.B >= 1 && p.T >= 1 && p.H >= 1 && p.cap >= 1, "%s: bad arguments", what);
    RST_REQUIRE(p.D == 64 || p.D == 128, "%s: head dim %d unsupported (64, 128)", what, p.D);
    RST_REQUIRE(p.T <= p.cap, "%s: %d new positions for a ring of capacity %d", what, p.T, p.cap);
    RST_REQUIRE(p.G >= 1 && p.H % p.G == 0, "%s: %d query heads are not a multiple of %d key/value heads", what, p.H, p.G);
    RST_REQUIRE(p.ldqkv >= (p.H + 2 * p.G) * p.D && p.ldqkv % 2 == 0, "%s: qkv row of %d floats for %d + 2 x %d heads of dim %d", what, p.ldqkv,
                p.H, p.G, p.D);
    RST_REQUIRE(p.rope_dims >= 0 && p.rope_dims <= p.D && p.rope_dims % 2 == 0, "%s: bad rope_dims %d", what, p.rope_dims);
    RST_REQUIRE(p.pos_stride == 0 || p.pos_stride == 1, "%s: position stride %ld (0: shared, 1: one per stream)", what, p.pos_stride);
    RST_REQUIRE(!p.lengths || (!attention && p.t0 >= 0), "%s: lengths belong to the append, with a chunk offset >= 0", what);
    if (attention) {
        RST_REQUIRE(p.out && p.q_rot && p.k_new && p.v_new, "%s: null output or workspace", what);
        RST_REQUIRE(p.window >= 1 && p.window <= p.cap, "%s: window %d for a ring of capacity %d", what, p.window, p.cap);
        RST_REQUIRE((long)p.B <= 65535 && p.H <= 65535, "%s: bad sizes", what);
    }
    return 0;
}

}  // namespace

long rst_lm_attn_prefill_workspace_bytes_impl(int B, int T, int H, int G, int D, int kv_bf16) {
    if (B < 1 || T < 1 || H < 1 || G < 1 || D < 1) return -1;
    return (long)B * T * H * D * 4 + 2 * (long)B * T * G * D * (kv_bf16 ? 2 : 4);
}

int rst_launch_lm_attn_prefill(const LmPrefillParams& p, hipStream_t stream) {
    if (const int rc = prefill_check(p, "lm_attn_prefill", true)) return rc;
    const long total = (long)p.B * p.T * (p.H + p.G) * (p.D / 2);
    const dim3 sgrid(cap_grid((total + 255) / 256, 4096));
    if (p.kv_bf16) {
        hipLaunchKernelGGL(stage_kernel<true>, sgrid, dim3(256), 0, stream, p, 0);
        const dim3 grid((p.T + 31) / 32, p.H, p.B);
        if (p.D == 64) hipLaunchKernelGGL(prefill_attn_bf16_kernel<64>, grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(prefill_attn_bf16_kernel<128>, grid, dim3(256), 0, stream, p);
        return rst_check_launch("lm_attn_prefill_kv16");
    }
    hipLaunchKernelGGL(stage_kernel<false>, sgrid, dim3(256), 0, stream, p, 0);
    const dim3 grid(p.T, p.H, p.B);
    if (p.D == 64) hipLaunchKernelGGL(prefill_attn_f32_kernel<64>, grid, dim3(64), 0, stream, p);
    else hipLaunchKernelGGL(prefill_attn_f32_kernel<128>, grid, dim3(64), 0, stream, p);
    return rst_check_launch("lm_attn_prefill");
}

int rst_launch_lm_ring_append(const LmPrefillParams& p, hipStream_t stream) {
    if (const int rc = prefill_check(p, "lm_ring_append", false)) return rc;
    const long total = (long)p.B * p.T * p.G * (p.D / 2);
    const dim3 sgrid(cap_grid((total + 255) / 256, 4096));
    if (p.kv_bf16) hipLaunchKernelGGL(stage_kernel<true>, sgrid, dim3(256), 0, stream, p, 1);
    else hipLaunchKernelGGL(stage_kernel<false>, sgrid, dim3(256), 0, stream, p, 1);
    return rst_check_launch("lm_ring_append");
}
