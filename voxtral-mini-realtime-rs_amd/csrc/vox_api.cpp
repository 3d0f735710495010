// vox_api.cpp -- C ABI of libvoxtral_hip.so (include/voxtral_hip.h): the model-forward
// orchestration (encoder, prefill, hipGraph-captured sync-free decode step), the batch drivers, the piecewise surface, the live streams.  Units of their own:
// the model loader (vox_model.cpp),
// the context and the audio front end's device side (vox_ctx.cpp), the Q4 operator boundary (vox_tensor.cpp), the decoder cache (vox_cache.cpp; vox_dev_base.h),
// the host arithmetic of the front end, the GGUF reader and the planners (vox_audio_host.cpp, vox_gguf.cpp, vox_batch_plan.cpp, vox_feed_plan.cpp; vox_host_base.h).
//
// Reference surface mirrored: src/audio/{io,pad,chunk,mel}.rs, src/gguf/{reader,tensor,op,linear,loader,model}.rs,
// src/models/time_embedding.rs.  No code is shared with oracle/ and there is no CPU fallback for compute.
#include "vox_page_pool.h"
#include "vox_dev_base.h"
#include "vox_snapshot.h"
#include "vox_kv_bf16.h"

#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <thread>
#include <vector>

using namespace vox;
using namespace vox_host;

namespace vox_host {
void binding_release(EngBinding& b) {
    for (void* p : {(void*)b.tab, (void*)b.part_val, (void*)b.part_idx}) if (p) (void)hipFree(p);
    if (b.err_word) (void)hipHostFree(b.err_word);
    b = EngBinding{};
}
}  // namespace vox_host
// the prefix itself, built here and nowhere else; static storage, so an upload from it has nothing to keep alive
static const struct PrefixTokens {
    int32_t t[VOX_PREFIX_TOKENS];
    PrefixTokens() { std::fill(t, t + VOX_PREFIX_TOKENS, VOX_TOK_STREAMING_PAD); t[0] = VOX_TOK_BOS; }
} PREFIX_TOKENS;

static int conv_len(int L) { return (L + 2 - 3) / 2 + 1; }   // models/layers/conv.rs:47-48

static int32_t ensure(float** p, size_t* cap, size_t need) {
    if (*cap >= need) return VOX_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIPCHK(hipMalloc((void**)p, need * sizeof(float))); *cap = need; return VOX_OK;
}

// ---- encoder + adapter (gguf/model.rs:425-434, 783-788) on device for n stacked utterances.
// Every utterance owns a budget of S_pad rows (S_pad = the longest S_enc rounded up to a multiple of the reshape factor, so the
// adapter's [S/4][4D] view of the stack stays uniformly strided); utterance i uses its first S_enc_i rows, the rest are
// scratch rows that flow through the row-independent operators and are never read by attention.  All GEMMs run once over
// the n*S_pad rows (the weights are streamed once per batch); convs are per utterance; attention is per utterance (grid.z).
// d_mels[i]: [n_mels][T[i]] device.  audio_out: [n][audio_rows][dec_dim] with audio_rows >= S_pad/4; S4_out[i] = S_enc_i / 4.
static int enc_rows(int T) { return conv_len(conv_len(T)); }
static int enc_row_budget(const vox_model* m, const int* T, int n) {
    int mx = 0; for (int i = 0; i < n; i++) mx = std::max(mx, enc_rows(T[i]));
    const int r = m->cfg.reshape_factor; return n == 1 ? mx : (mx + r - 1) / r * r;
}
// conv stem (models/layers/conv.rs:78-83, gguf/model.rs:426-427): d_mel [n_mels][T] -> x [S][enc_dim] token-major; c1 = scratch of c1_floats(T) floats
static size_t conv_scratch_floats(const vox_model* m, int T) {
    const int D = m->cfg.enc_dim, T1 = conv_len(T);
    return std::max((size_t)D * T1, (size_t)(T + 2) * m->cfg.n_mels + (size_t)(T1 + 2) * D) + 64;   // VALU conv: [D][T1]; MFMA conv: padded token-major mel + conv1 output
}
static int32_t conv_stem_dev(vox_model* m, const float* d_mel, int T, float* c1, float* x) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream; const int D = c.enc_dim, T1 = conv_len(T), S = conv_len(T1);
    const bool conv_mfma = m->conv1_g.qs && m->conv2_g.qs && !knob_str("VOX_CONV_VALU");
    if (conv_mfma) {
        // gelu(conv1d k3 s2 p1) as an im2col GEMM: with the input token-major and one zero row either side, output row t reads the
        // CONTIGUOUS window rows [2t, 2t+2] of the padded buffer (= frames 2t-1..2t+1): A = that buffer with row stride 2*Cin, K = 3*Cin
        const int Cm = c.n_mels;
        float* melT = c1; float* c1T = melT + (size_t)(T + 2) * Cm;                       // [(T+2)][Cm], [(T1+2)][D]
        HIPCHK(hipMemsetAsync(melT, 0, (size_t)Cm * 4, s)); HIPCHK(hipMemsetAsync(melT + (size_t)(T + 1) * Cm, 0, (size_t)Cm * 4, s));
        HIPCHK(hipMemsetAsync(c1T, 0, (size_t)D * 4, s)); HIPCHK(hipMemsetAsync(c1T + (size_t)(T1 + 1) * D, 0, (size_t)D * 4, s));
        HIPCHK(launch_transpose(d_mel, Cm, T, melT + Cm, s));                          // [Cm][T] -> [T][Cm]
        { GemmParams g{}; g.w = m->conv1_g; g.x = melT; g.x_stride = 2 * Cm; g.M = T1; g.out = c1T + D; g.out_stride = D; g.bias = m->conv1_b; HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
        { GemmParams g{}; g.w = m->conv2_g; g.x = c1T; g.x_stride = 2 * D; g.M = S; g.out = x; g.out_stride = D; g.bias = m->conv2_b; HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
    } else {
        HIPCHK(launch_conv1d_gelu(d_mel, c.n_mels, T, m->conv1_w, m->conv1_b, D, c1, 0, s));
        HIPCHK(launch_conv1d_gelu(c1, D, T1, m->conv2_w, m->conv2_b, D, x, 1, s));      // token-major [S][D] (swap_dims, model.rs:427)
    }
    return VOX_OK;
}
// PACKED form (audio_off_out != nullptr; the continuous batch): no utterance is padded to the longest of the stack -- utterance i owns rp_i = S_enc_i rounded up to a multiple
// of the reshape factor (>= 4 * 40) rows, back to back; RoPE takes the position of every row from a table, attention the start row of every utterance (AttnParams::
// seq_row_off), the adapter's [rows / 4][4 D] view stays aligned because every start row is a multiple of 4.  audio_out receives packed_rows / 4 rows; audio_off_out[i] =
// the float offset of utterance i's first row.  A ragged stack costs its own frames, not n x the longest (a rank's 64 longest clips of the FLEURS-like corpus span 9 .. 30 s:
// 401 ms padded, profiles/r05_continuous_sweep.txt).
static int enc_packed_rows_of(const vox_model* m, int T) { const int R = m->cfg.reshape_factor; return std::max((enc_rows(T) + R - 1) / R * R, R * 40); }
static long enc_packed_rows(const vox_model* m, const int* T, int n) { long r = 0; for (int i = 0; i < n; i++) r += enc_packed_rows_of(m, T[i]); return r; }
// which forms a stack took (vox_debug_encode_batch): stacked rows, w2 / wo split-K slice counts (0 = unsplit), q|k|v launches with RoPE in the GEMM's epilogue
struct EncForms { long Mtot = 0; int ksp = 0, ksp_wo = 0, fused_rope = 0; };
// prefix_rows = r0 > 0 (one utterance, unpacked; a multiple of the reshape factor): rows [0, r0) of every layer are NOT computed -- their keys and values come from the
// model's prefix state (m->pfx.enc_kv, the attention kernel's second K / V segment), the conv stem still runs over the whole clip (two launches; its symmetric padding is
// why the mel is not simply cut), the layers carry rows r0 .. S-1 at RoPE positions r0 .., the adapter writes audio rows r0 / R .. and leaves the rows before them alone.
static int32_t encode_batch_dev(vox_model* m, int n, const float* const* d_mels, const int* T, float* audio_out, int audio_rows, int* S4_out, long* audio_off_out = nullptr,
                                EncForms* forms = nullptr, int prefix_rows = 0) {
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const int D = c.enc_dim, H = c.enc_heads, hd = c.enc_head_dim, QD = H * hd, F = c.enc_ffn, R = c.reshape_factor;
    const bool packed = audio_off_out != nullptr;
    ARGCHK(n <= 128, "internal: encoder stack of %d utterances", n);
    const int S_pad = enc_row_budget(m, T, n);
    int T1max = 0; bool any = false;
    std::vector<int> S(n);
    for (int i = 0; i < n; i++) { S[i] = enc_rows(T[i]); S4_out[i] = S[i] / R; T1max = std::max(T1max, conv_len(T[i])); any = any || S4_out[i] > 0; }
    if (!any || S_pad <= 0) return VOX_OK;
    ARGCHK(S_pad <= m->enc_rope_len, "audio too long for the encoder RoPE table (%d > %d positions); chunk it (--max-mel-frames)", S_pad, m->enc_rope_len);
    std::vector<int> roff(n + 1, 0);      // packed: first row of every utterance
    if (packed) for (int i = 0; i < n; i++) roff[i + 1] = roff[i] + enc_packed_rows_of(m, T[i]);
    const int r0 = prefix_rows;
    ARGCHK(r0 == 0 || (n == 1 && !packed && r0 % R == 0 && r0 < S_pad && m->pfx.enc_built && r0 == m->pfx.RC), "internal: encoder prefix of %d rows", r0);
    const int Mfull = packed ? roff[n] : n * S_pad;                  // rows the conv stems write
    const int Mtot = Mfull - r0, M4 = packed ? Mtot / R : n == 1 ? S4_out[0] - r0 / R : Mtot / R;          // rows the layers carry; adapter rows
    ARGCHK(!m->pfx.capture || (n == 1 && !packed && r0 == 0 && m->pfx.capture_rows <= S_pad), "internal: prefix capture");
    ARGCHK(packed || n == 1 || audio_rows >= S_pad / R, "internal: audio row budget %d < %d", audio_rows, S_pad / R);
    int Tmax = 0; for (int i = 0; i < n; i++) Tmax = std::max(Tmax, T[i]);
    (void)T1max;
    const size_t c1_floats = conv_scratch_floats(m, Tmax);
    // w2 (N = D columns only, K = F: 40 K-steps per workgroup at 250 workgroups for one clip) as a split-K GEMM: four K slices -> four partial planes, summed (fixed
    // order) by the NEXT RMSNorm together with the residual add.  Only while the unsplit grid leaves the chip underfilled; VOX_ENC_SPLITK=0 switches it off.
    int ksp = 0;
    {
        const Q4W& w2 = m->enc[0].w2.w;
        const long wgs = (long)((w2.N + 127) / 128) * ((Mtot + 31) / 32);
        const bool geom_ok = w2.fmt == WFMT_Q4_0 && w2.qt && w2.st && w2.nb % 16 == 0 && Mtot > 48 && D % 4 == 0 && D <= 4096;      // what the split-K GEMM + summing norm can run at all
        if (geom_ok && wgs < 1024) ksp = 4;
        if (const char* e = knob_str("VOX_ENC_SPLITK")) ksp = geom_ok && atoi(e) > 1 ? std::min(atoi(e), w2.nb / 4) : 0;      // the knob picks the slice count on an eligible geometry, it never forces an ineligible one
        for (int l = 0; ksp && l < c.enc_layers; l++) if (m->enc[l].w2.w.fmt != WFMT_Q4_0 || !m->enc[l].w2.w.qt || m->enc[l].w2.w.nb / 4 < ksp) ksp = 0;
    }
    int ksp_wo = ksp ? 2 : 0;      // the same for wo (K = QD: 10 K-steps), two slices (7.85 -> 7.76 ms per clip; four: 7.93; profiles/r03_enc_splitk.txt); VOX_ENC_SPLITK_WO overrides
    if (ksp) { if (const char* e = knob_str("VOX_ENC_SPLITK_WO")) ksp_wo = atoi(e) > 1 ? std::min(atoi(e), ksp) : 0; }
    for (int l = 0; ksp_wo && l < c.enc_layers; l++) if (m->enc[l].wo.w.fmt != WFMT_Q4_0 || !m->enc[l].wo.w.qt || m->enc[l].wo.w.nb / 4 < ksp_wo || m->enc[l].wo.w.nb % 4) ksp_wo = 0;
    const size_t need = c1_floats + (size_t)Mfull * D + (size_t)Mtot * D + (size_t)Mtot * QD * 4 + (size_t)Mtot * F + (size_t)(M4 + 1) * m->ad0.w.N + (size_t)ksp * Mtot * D + 1024;
    VOXCHK(ensure(&m->ws, &m->ws_floats, need));
    if (forms) { forms->Mtot = Mtot; forms->ksp = ksp; forms->ksp_wo = ksp_wo; forms->fused_rope = 0; }
    float* c1 = m->ws; float* x0 = c1 + c1_floats / 64 * 64; float* x = x0 + (size_t)r0 * D; float* xn = x0 + (size_t)Mfull * D; float* qkv = xn + (size_t)Mtot * D;      // x0: the conv stem's rows; x: the first row the layers carry
    float* att = qkv + (size_t)Mtot * QD * 3; float* ffn = att + (size_t)Mtot * QD; float* ah = ffn + (size_t)Mtot * F; float* w2p = ah + (size_t)(M4 + 1) * m->ad0.w.N;
    const int* d_len = nullptr; const int* d_roff = nullptr; const int* d_rpos = nullptr;
    if (n > 1 || packed) {
        HIPCHK(hipMemsetAsync(x, 0, (size_t)Mtot * D * 4, s));               // scratch rows: finite values
        HIPCHK(hipMemsetAsync(att, 0, (size_t)Mtot * QD * 4, s));            // rows >= seq_len[i] are never written by attention
        if (!m->d_seq_len) HIPCHK(hipMalloc((void**)&m->d_seq_len, 128 * sizeof(int)));
        m->h_seq_len.assign(S.begin(), S.end());
        HIPCHK(hipMemcpyAsync(m->d_seq_len, m->h_seq_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        d_len = m->d_seq_len;
    }
    if (packed) {      // start rows and the position of every row (host-built, uploaded behind the stream; the host vectors are model members: they outlive the copies)
        if (!m->d_seq_off) HIPCHK(hipMalloc((void**)&m->d_seq_off, 128 * sizeof(int)));
        if (m->row_pos_cap < (size_t)Mtot) { if (m->d_row_pos) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipFree(m->d_row_pos)); } m->d_row_pos = nullptr; m->row_pos_cap = 0;
                                              HIPCHK(hipMalloc((void**)&m->d_row_pos, (size_t)Mtot * sizeof(int))); m->row_pos_cap = (size_t)Mtot; }
        HIPCHK(hipStreamSynchronize(s));      // (the previous stack's copies out of these host vectors have completed)
        m->h_seq_off.assign(roff.begin(), roff.begin() + n); m->h_row_pos.resize((size_t)Mtot);
        for (int i = 0; i < n; i++) for (int r = roff[i]; r < roff[i + 1]; r++) m->h_row_pos[(size_t)r] = std::min(r - roff[i], m->enc_rope_len - 1);
        HIPCHK(hipMemcpyAsync(m->d_seq_off, m->h_seq_off.data(), (size_t)n * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(m->d_row_pos, m->h_row_pos.data(), (size_t)Mtot * 4, hipMemcpyHostToDevice, s));
        d_roff = m->d_seq_off; d_rpos = m->d_row_pos;
    }
    for (int i = 0; i < n; i++) {
        if (S[i] <= 0) continue;
        VOXCHK(conv_stem_dev(m, d_mels[i], T[i], c1, x0 + (packed ? (size_t)roff[i] : (size_t)i * S_pad) * D));
    }
    const int seq_rows = packed ? 0 : n > 1 ? S_pad : 0;
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayer& L = m->enc[l];
        if (ksp && l > 0) HIPCHK(launch_rms_norm_sumk(x, D, Mtot, D, w2p, (size_t)Mtot * D, ksp, L.attn_norm, c.norm_eps, xn, D, s));      // + the previous layer's w2
        else HIPCHK(launch_rms_norm(x, D, Mtot, D, L.attn_norm, nullptr, c.norm_eps, xn, D, s));
        if (Mtot > 48) {      // q|k|v with RoPE on the q and k columns: in the large-M GEMM's epilogue where that kernel runs, else store + rope_kernel (launch_q4_gemm, EPI_ROPE_ROWS)
            GemmParams g{}; g.w = L.wqkv.w; g.x = xn; g.x_stride = D; g.M = Mtot; g.out = qkv; g.out_stride = 3 * QD; g.bias = L.wqkv.bias;
            g.rope_cos = m->enc_cos + (size_t)r0 * (hd / 2); g.rope_sin = m->enc_sin + (size_t)r0 * (hd / 2);      // row i sits at position r0 + i: the tables are [position][hd / 2]
            g.hd = hd; g.n_q = 2 * QD; g.pos = d_rpos; g.rope_seq_rows = seq_rows;
            bool fused = false; HIPCHK(launch_q4_gemm(g, EPI_ROPE_ROWS, s, &fused));
            if (forms && fused) forms->fused_rope++;
        } else {
            VOXCHK(q4_linear_dev(cx, L.wqkv.w, L.wqkv.bias, xn, D, Mtot, qkv, 3 * QD));
            HIPCHK(launch_rope(qkv, Mtot, 3 * QD, 2 * QD, hd, r0, m->enc_cos, m->enc_sin, s, seq_rows, d_rpos));
        }
        if (m->pfx.capture)      // building the prefix state: this layer's k | v rows 0 .. capture_rows-1
            HIPCHK(hipMemcpy2DAsync(m->pfx.capture + (size_t)l * m->pfx.capture_rows * 2 * QD, (size_t)2 * QD * 4, qkv + QD, (size_t)3 * QD * 4, (size_t)2 * QD * 4, (size_t)m->pfx.capture_rows,
                                    hipMemcpyDeviceToDevice, s));
        AttnParams ap{}; ap.q = qkv; ap.q_stride = 3 * QD; ap.k = qkv + QD; ap.v = qkv + 2 * QD; ap.kv_row_stride = 3 * QD; ap.kv_head_stride = hd;
        ap.out = att; ap.out_stride = QD; ap.M = S_pad - r0; ap.kv_len = S_pad; ap.n_heads = H; ap.n_kv_heads = H; ap.offset = r0; ap.window = c.enc_window;
        if (r0) { ap.prefix_k = m->pfx.enc_kv + (size_t)l * r0 * 2 * QD; ap.prefix_v = ap.prefix_k + QD; ap.prefix_len = r0; ap.prefix_row_stride = 2 * QD; ap.prefix_head_stride = hd; }
        ap.seq_len = d_len; ap.q_seq_stride = S_pad * 3 * QD; ap.out_seq_stride = S_pad * QD; ap.kv_seq_stride = (long)S_pad * 3 * QD; ap.seq_row_off = d_roff;
        HIPCHK(launch_attn_prefill(ap, hd, s, n));
        if (ksp_wo) {      // (w2p is free here: the previous layer's w2 planes were consumed by this layer's first norm)
            VOXCHK(q4_linear_dev(cx, L.wo.w, L.wo.bias, att, QD, Mtot, w2p, D, EPI_STORE, nullptr, 0, ksp_wo));
            HIPCHK(launch_rms_norm_sumk(x, D, Mtot, D, w2p, (size_t)Mtot * D, ksp_wo, L.ffn_norm, c.norm_eps, xn, D, s));
        } else {
            VOXCHK(q4_linear_dev(cx, L.wo.w, L.wo.bias, att, QD, Mtot, x, D, EPI_RESID, x, D));
            HIPCHK(launch_rms_norm(x, D, Mtot, D, L.ffn_norm, nullptr, c.norm_eps, xn, D, s));
        }
        VOXCHK(q4_linear_dev(cx, L.w13.w, nullptr, xn, D, Mtot, ffn, F, EPI_SWIGLU));
        if (ksp) VOXCHK(q4_linear_dev(cx, L.w2.w, L.w2.bias, ffn, F, Mtot, w2p, D, EPI_STORE, nullptr, 0, ksp));
        else VOXCHK(q4_linear_dev(cx, L.w2.w, L.w2.bias, ffn, F, Mtot, x, D, EPI_RESID, x, D));
    }
    if (ksp && c.enc_layers > 0) HIPCHK(launch_rms_norm_sumk(x, D, Mtot, D, w2p, (size_t)Mtot * D, ksp, m->enc_norm, c.norm_eps, xn, D, s));
    else HIPCHK(launch_rms_norm(x, D, Mtot, D, m->enc_norm, nullptr, c.norm_eps, xn, D, s));
    // reshape_encoder_output (models/adapter.rs:108-122): rows [0, 4*S4) of each utterance viewed as [S4][4D]; adapter (model.rs:745-749)
    VOXCHK(q4_linear_dev(cx, m->ad0.w, nullptr, xn, D * R, M4, ah, m->ad0.w.N, EPI_GELU));
    if (packed) { for (int i = 0; i < n; i++) audio_off_out[i] = (long)(roff[i] / R) * c.dec_dim; }
    if (packed || n == 1 || audio_rows * R == S_pad) VOXCHK(q4_linear_dev(cx, m->ad2.w, nullptr, ah, m->ad0.w.N, M4, audio_out + (size_t)(r0 / R) * c.dec_dim, c.dec_dim));
    else for (int i = 0; i < n; i++)      // wider per-utterance stride on the output side
        VOXCHK(q4_linear_dev(cx, m->ad2.w, nullptr, ah + (size_t)i * (S_pad / R) * m->ad0.w.N, m->ad0.w.N, S_pad / R, audio_out + (size_t)i * audio_rows * c.dec_dim, c.dec_dim));
    return VOX_OK;
}
static int32_t encode_dev(vox_model* m, const float* d_mel, int T, int* S4_out, int prefix_rows = 0) {
    const int S4 = enc_rows(T) / m->cfg.reshape_factor;
    if (S4 > 0) { size_t cap = (size_t)m->audio_cap * m->cfg.dec_dim; VOXCHK(ensure(&m->d_audio, &cap, (size_t)S4 * m->cfg.dec_dim)); m->audio_cap = (int)(cap / m->cfg.dec_dim); }
    return encode_batch_dev(m, 1, &d_mel, &T, m->d_audio, S4, S4_out, nullptr, nullptr, prefix_rows);
}

// ---- streaming encoder: Q4AudioEncoder::create_cache / forward_with_cache (gguf/model.rs:437-459), Q4EncoderLayer::forward_with_cache
// (:299-317), Q4Attention::forward_with_cache (:125-174), Q4VoxtralModel::encode_audio_with_cache (:791-799), eviction KVCache::apply_sliding_window
// (kv_cache.rs:176-203).  One cache = K / V rows [enc_layers][enc_heads][capacity][64] f32.  A chunk's K / V are appended at row `len`; when the chunk
// does not fit, the cache is compacted to its last `enc_window` rows first (keys older than the window can never be attended again: exact).  RoPE uses
// the ABSOLUTE stream position (abs_pos), so chunked == whole-utterance for the transformer stack at any stream length.
extern "C" int32_t vox_encoder_cache_create(vox_model* m, int32_t capacity_rows, vox_cache** out) {
    ARGCHK(m && out, "null argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg;
    if (capacity_rows <= 0) capacity_rows = 2 * c.enc_window + 512;
    ARGCHK(capacity_rows > c.enc_window, "encoder cache capacity %d must exceed the sliding window (%d)", capacity_rows, c.enc_window);
    vox_cache* k = new vox_cache(); k->m = m; k->ctx = m->ctx; k->max_seq = capacity_rows; k->kind = 1;
    const size_t n = (size_t)c.enc_layers * c.enc_heads * capacity_rows * c.enc_head_dim * 4;
    if (hipMalloc((void**)&k->k, n) != hipSuccess || hipMalloc((void**)&k->v, n) != hipSuccess) { if (k->k) (void)hipFree(k->k); delete k; return fail(VOX_ERR_HIP, "hipMalloc of encoder KV cache failed"); }
    HIPCHK(hipMemsetAsync(k->k, 0, n, m->ctx->stream)); HIPCHK(hipMemsetAsync(k->v, 0, n, m->ctx->stream));
    k->layer_stride = (size_t)c.enc_heads * capacity_rows * c.enc_head_dim;
    cache_register(k);
    *out = k; return VOX_OK;
}
extern "C" int32_t vox_cache_abs_pos(const vox_cache* k, int32_t* out) { ARGCHK(k && out, "null argument"); *out = k->kind == 1 ? k->abs_pos : k->len; return VOX_OK; }

// keep the last `keep` rows of every (layer, head) plane: rows [len - keep, len) -> [0, keep).  Two strided 2-D copies through the workspace
// (source and destination ranges may overlap).  One pitch covers all planes: layer_stride == heads * capacity * hd.
static int32_t enc_cache_evict(vox_model* m, vox_cache* kc, int keep) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (keep >= kc->len) return VOX_OK;
    const size_t planes = (size_t)c.enc_layers * c.enc_heads, pitch = (size_t)kc->max_seq * c.enc_head_dim * 4, width = (size_t)keep * c.enc_head_dim * 4;
    VOXCHK(ensure(&m->ws, &m->ws_floats, planes * width / 4 + 64));
    for (float* base : {kc->k, kc->v}) {
        const char* src = reinterpret_cast<const char*>(base) + (size_t)(kc->len - keep) * c.enc_head_dim * 4;
        HIPCHK(hipMemcpy2DAsync(m->ws, width, src, pitch, width, planes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(base, pitch, m->ws, width, width, planes, hipMemcpyDeviceToDevice, s));
    }
    kc->len = keep;
    return VOX_OK;
}
extern "C" int32_t vox_encoder_cache_apply_sliding_window(vox_cache* kc, int32_t window) {      // kv_cache.rs:176-203, all layers
    ARGCHK(kc && kc->kind == 1 && window > 0, "bad argument"); VOXCHK(ctx_bind(kc->ctx));
    VOXCHK(enc_cache_evict(kc->m, kc, window)); HIPCHK(hipStreamSynchronize(kc->ctx->stream)); return VOX_OK;
}

// the 65 536-position RoPE table of the streaming encoder (the load-time table's formula, models/layers/rope.rs:35-64), built at first use
static int32_t enc_stream_rope_ensure(vox_model* m) {
    if (m->enc_cos_s) return VOX_OK;
    const vox_model_cfg& c = m->cfg; const int hd = c.enc_head_dim;
    const int len = ROPE_ENC_STREAM_TABLE_LEN, half = hd / 2; std::vector<float> ct((size_t)len * half), st((size_t)len * half);
    rope_rows_fill(hd, c.rope_theta, 0, len, len, nullptr, ct.data(), st.data());
    HIPCHK(hipMalloc((void**)&m->enc_cos_s, ct.size() * 4)); HIPCHK(hipMalloc((void**)&m->enc_sin_s, st.size() * 4));
    HIPCHK(hipMemcpy(m->enc_cos_s, ct.data(), ct.size() * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(m->enc_sin_s, st.data(), st.size() * 4, hipMemcpyHostToDevice));
    m->enc_rope_s_len = len;
    return VOX_OK;
}
static int32_t encode_with_cache_dev(vox_model* m, const float* d_mel, int T, vox_cache* kc, int* S4_out) {
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const int D = c.enc_dim, H = c.enc_heads, hd = c.enc_head_dim, QD = H * hd, F = c.enc_ffn, R = c.reshape_factor;
    const int S = enc_rows(T), S4 = S / R; *S4_out = S4;
    if (S <= 0) return VOX_OK;
    ARGCHK(S <= kc->max_seq - std::min(c.enc_window, kc->max_seq - 1), "chunk of %d encoder rows does not fit a cache of %d rows next to the %d-row window", S, kc->max_seq, c.enc_window);
    if (kc->len + S > kc->max_seq) VOXCHK(enc_cache_evict(m, kc, std::min(kc->len, c.enc_window)));
    // RoPE table for absolute stream positions (the load-time table covers 4096 rows, gguf/loader.rs:196-198)
    const float *cos_t = m->enc_cos, *sin_t = m->enc_sin;
    if (kc->abs_pos + S > m->enc_rope_len) {
        VOXCHK(enc_stream_rope_ensure(m));
        ARGCHK(kc->abs_pos + S <= m->enc_rope_s_len, "stream of %d encoder positions exceeds the streaming RoPE table (%d)", kc->abs_pos + S, m->enc_rope_s_len);
        cos_t = m->enc_cos_s; sin_t = m->enc_sin_s;
    }
    if (S4 > 0) { size_t cap = (size_t)m->audio_cap * c.dec_dim; VOXCHK(ensure(&m->d_audio, &cap, (size_t)S4 * c.dec_dim)); m->audio_cap = (int)(cap / c.dec_dim); }
    const size_t c1f = conv_scratch_floats(m, T);
    const size_t need = c1f + (size_t)S * D * 2 + (size_t)S * QD * 4 + (size_t)S * F + (size_t)(S4 + 1) * m->ad0.w.N + 1024;
    VOXCHK(ensure(&m->ws, &m->ws_floats, need));
    float* c1 = m->ws; float* x = c1 + c1f / 64 * 64; float* xn = x + (size_t)S * D; float* qkv = xn + (size_t)S * D;
    float* att = qkv + (size_t)S * QD * 3; float* ffn = att + (size_t)S * QD; float* ah = ffn + (size_t)S * F;
    VOXCHK(conv_stem_dev(m, d_mel, T, c1, x));
    const int off = kc->len; const size_t lf = kc->layer_stride;
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayer& L = m->enc[l]; float* kl = kc->k + (size_t)l * lf; float* vl = kc->v + (size_t)l * lf;
        HIPCHK(launch_rms_norm(x, D, S, D, L.attn_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, L.wqkv.w, L.wqkv.bias, xn, D, S, qkv, 3 * QD));
        HIPCHK(launch_rope(qkv, S, 3 * QD, 2 * QD, hd, kc->abs_pos, cos_t, sin_t, s, 0));                     // q and k at the absolute positions
        HIPCHK(launch_kv_store(qkv, S, 3 * QD, QD, H, hd, off, kl, vl, kc->max_seq * hd, s));                   // append at rows [len, len + S)
        AttnParams ap{}; ap.q = qkv; ap.q_stride = 3 * QD; ap.k = kl; ap.v = vl; ap.kv_row_stride = hd; ap.kv_head_stride = kc->max_seq * hd;
        ap.out = att; ap.out_stride = QD; ap.M = S; ap.kv_len = off + S; ap.n_heads = H; ap.n_kv_heads = H; ap.offset = off; ap.window = c.enc_window;
        HIPCHK(launch_attn_prefill(ap, hd, s, 1));
        VOXCHK(q4_linear_dev(cx, L.wo.w, L.wo.bias, att, QD, S, x, D, EPI_RESID, x, D));
        HIPCHK(launch_rms_norm(x, D, S, D, L.ffn_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, L.w13.w, nullptr, xn, D, S, ffn, F, EPI_SWIGLU));
        VOXCHK(q4_linear_dev(cx, L.w2.w, L.w2.bias, ffn, F, S, x, D, EPI_RESID, x, D));
    }
    kc->len = off + S; kc->abs_pos += S;
    if (S4 > 0) {
        HIPCHK(launch_rms_norm(x, D, S4 * R, D, m->enc_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, m->ad0.w, nullptr, xn, D * R, S4, ah, m->ad0.w.N, EPI_GELU));
        VOXCHK(q4_linear_dev(cx, m->ad2.w, nullptr, ah, m->ad0.w.N, S4, m->d_audio, c.dec_dim));
    }
    return VOX_OK;
}
extern "C" int32_t vox_encode_audio_with_cache(vox_model* m, const float* mel, int32_t T, vox_cache* enc_cache, float* out, int32_t cap_rows, int32_t* S,
                                               int32_t mem_kind) {
    ARGCHK(m && mel && enc_cache && out && S, "null argument"); ARGCHK(T > 0, "empty mel");
    ARGCHK(enc_cache->kind == 1 && enc_cache->m == m, "not an encoder cache of this model (vox_encoder_cache_create)"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    ARGCHK(cap_rows >= enc_rows(T) / c.reshape_factor, "output capacity %d rows < %d", cap_rows, enc_rows(T) / c.reshape_factor);      // BEFORE the chunk's K / V are appended: a refused call leaves the stream cache untouched
    const float* d_mel = mel;
    if (mem_kind == VOX_MEM_HOST) {
        VOXCHK(ensure(&m->d_mel, &m->mel_cap, (size_t)c.n_mels * T));
        HIPCHK(hipMemcpyAsync(m->d_mel, mel, (size_t)c.n_mels * T * 4, hipMemcpyHostToDevice, s)); d_mel = m->d_mel;
    }
    int S4 = 0; VOXCHK(encode_with_cache_dev(m, d_mel, T, enc_cache, &S4));
    if (S4 > 0) HIPCHK(hipMemcpyAsync(out, m->d_audio, (size_t)S4 * c.dec_dim * 4, mem_kind == VOX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    *S = S4; return VOX_OK;
}

// ---- multi-row decoder forward (prefill): x [M][D] device, in place; positions off..off+M-1  (gguf/model.rs:370-387).
// n_seq > 1: x holds n_seq stacked sequences of seq_rows = M / n_seq rows, each with its own cache slice kv_seq_stride floats apart
// (positions restart at off per sequence); the GEMMs run once over all M rows.
// A layer keeps f32 rows between its launches, or -- 17..48 rows in one sequence (the 38-token prefill) -- both RMSNorms write their output straight as XF tiles (the MFMA
// A-fragments the q4_skinny_mt_kernel consumes) into the context's XF scratch: no f32 xn, no conversion launch for q|k|v and w1|w3.  A GEMM on XF tiles may leave K-slice
// planes in the context's plane buffer for the launch behind it to sum.  plan_prefill decides every layer's form, operator by operator; decoder_prefill_dev runs it.
struct PrefillLayerForm {
    enum Qkv : uint8_t { QKV_F32, QKV_XF, QKV_PLANES } qkv = QKV_F32;              // f32 rows | XF tiles, launch_q4_gemm | planes, their finish also applies RoPE and writes the k / v rows into the cache (three launches less)
    enum Wo : uint8_t { WO_F32, WO_PLANES_ROWS, WO_PLANES_XF } wo = WO_F32;        // f32 rows | planes of the f32 attention rows (xf_rows) | of the XF tiles the short-sequence attention leaves; the RMSNorm behind sums them (one launch less)
    enum W13 : uint8_t { W13_F32, W13_XF, W13_PLANES } w13 = W13_F32;              // f32 rows | XF tiles, launch_q4_gemm | planes, their finish writes SiLU(gate) * up straight into the XF tiles w2 reads (no f32 activations, no conversion launch)
    enum W2 : uint8_t { W2_F32, W2_PLANES_ROWS, W2_PLANES_XF } w2 = W2_F32;        // f32 rows | planes of the f32 activations (xf_rows) | of the w1|w3 finish's XF tiles; the NEXT layer's first RMSNorm sums them
    int kz_qkv = 0, kz_wo = 0, kz_13 = 0, kz_w2 = 0;      // K slices of the operator's planes
    bool f32_rows() const { return qkv == QKV_F32 && wo == WO_F32 && w13 == W13_F32 && w2 == W2_F32; }
    // Invariants: kz_x != 0 exactly when operator x is a planes form.  The norm that sums wo's planes writes XF tiles only: wo as planes -> w1|w3 not on f32 rows.  The w1|w3 finish
    // needs that norm in front and leaves XF tiles only: W13_PLANES -> wo as planes, and W13_PLANES <-> W2_PLANES_XF.  w2's planes wait for an XF norm: `prev`->w2 as planes -> qkv not
    // on f32 rows (a finishing kernel sums the last layer's).
    bool valid(const PrefillLayerForm* prev) const {
        return (kz_qkv != 0) == (qkv == QKV_PLANES) && (kz_wo != 0) == (wo != WO_F32) && (kz_13 != 0) == (w13 == W13_PLANES) && (kz_w2 != 0) == (w2 != W2_F32) && (wo == WO_F32 || w13 != W13_F32) &&
               (w13 != W13_PLANES || wo != WO_F32) && (w13 == W13_PLANES) == (w2 == W2_PLANES_XF) && (!prev || prev->w2 == W2_F32 || qkv != QKV_F32);
    }
};
// A prefill layer's attention launch but for its pointers and kv_seq_stride: plan_prefill asks attn_prefill_small_ok about what decoder_prefill_dev launches
static AttnParams prefill_attn_params(const vox_model_cfg& c, int max_seq, int M, int n_seq, int off) {
    const int hd = c.dec_head_dim, QD = c.dec_heads * hd, W = QD + 2 * c.dec_kv_heads * hd, seq_rows = n_seq > 1 ? M / n_seq : 0, Mq = n_seq > 1 ? seq_rows : M;
    AttnParams ap{}; ap.q_stride = W; ap.kv_row_stride = hd; ap.kv_head_stride = max_seq * hd; ap.out_stride = QD; ap.M = Mq; ap.kv_len = off + Mq; ap.n_heads = c.dec_heads;
    ap.n_kv_heads = c.dec_kv_heads; ap.offset = off; ap.window = c.dec_window; ap.q_seq_stride = seq_rows * W; ap.out_seq_stride = seq_rows * QD;
    return ap;
}
// Every layer's form for one call; launches nothing.  Asks the context for the XF scratch when the call's shape and knobs allow XF tiles at all and for the plane buffer when planes
// may be used, and decides on what it got; eligibility is per layer (a checkpoint may mix tensor formats).  Cross-check knobs: VOX_PREFILL_NO_NORM_XF, VOX_NO_SKINNY_MT (the GEMMs
// on f32 rows): every layer on f32 rows; VOX_PREFILL_NO_SUMK: no planes (finishing kernels inside launch_q4_gemm instead); VOX_PREFILL_NO_FUSED_FIN: no QKV_PLANES, W13_PLANES, W2_PLANES_XF.
static std::vector<PrefillLayerForm> plan_prefill(vox_model* m, int M, int n_seq, int off, int max_seq) {
    using PF = PrefillLayerForm;
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx;
    const int D = c.dec_dim, hd = c.dec_head_dim, QD = c.dec_heads * hd, W = QD + 2 * c.dec_kv_heads * hd, F = c.dec_ffn;
    const bool no_norm_xf = knob_str("VOX_PREFILL_NO_NORM_XF"), no_skinny_mt = knob_str("VOX_NO_SKINNY_MT"), no_sumk = knob_str("VOX_PREFILL_NO_SUMK"), no_fused_fin = knob_str("VOX_PREFILL_NO_FUSED_FIN");
    std::vector<PF> forms(c.dec_layers);      // every operator on f32 rows
    if (n_seq != 1 || M <= 16 || M > 48 || no_norm_xf || no_skinny_mt) return forms;
    cx->want_scratch(true, false);
    if (!cx->xf_scratch) return forms;
    if (!no_sumk) cx->want_scratch(false, true);
    const bool planes = !no_sumk && cx->kz_scratch, fin = planes && !no_fused_fin;      // planes summed by the norms | also the finishing kernels of q|k|v and w1|w3
    auto xf_ok = [&](const Q4W& w) { return w.fmt == WFMT_Q4_0 && w.qt && w.st && w.nb % 4 == 0 && w.K == D && D % 128 == 0 && D <= 10240; };
    auto kz_fits = [&](int kz, int N) { return (size_t)kz * M * N * 4 <= cx->kz_scratch_bytes; };
    auto xf_fits = [&](int K) { return (size_t)((M + 15) / 16) * K * 64 <= cx->xf_scratch_bytes; };
    // round 6: a short sequence from position 0 (the 38-token prefill) takes the short-sequence attention kernel, whose rows leave as the XF tiles the wo GEMM reads
    // (no f32 round trip, no xf_rows launch) when that GEMM is the planes form
    const bool att_xf = xf_fits(QD) && attn_prefill_small_ok(prefill_attn_params(c, max_seq, M, n_seq, off), hd, n_seq);
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayer& L = m->dec[l]; PF& f = forms[l];
        if (xf_ok(L.wqkv.w)) {
            f.kz_qkv = fin ? q4_skinny_mt2_plan(L.wqkv.w, M) : 0; if (!kz_fits(f.kz_qkv, W)) f.kz_qkv = 0;
            f.qkv = f.kz_qkv ? PF::QKV_PLANES : PF::QKV_XF;
        }
        const bool w13_xf = xf_ok(L.w13.w);
        f.kz_wo = planes && w13_xf && L.wo.w.N == D && QD % 128 == 0 ? q4_skinny_mt2_plan(L.wo.w, M) : 0; if (!kz_fits(f.kz_wo, D)) f.kz_wo = 0;
        if (f.kz_wo) f.wo = att_xf ? PF::WO_PLANES_XF : PF::WO_PLANES_ROWS;
        f.kz_w2 = planes && L.w2.w.N == D && F % 128 == 0 && F <= 16384 ? q4_skinny_mt2_plan(L.w2.w, M) : 0;
        if (!kz_fits(f.kz_w2, D) || !(l + 1 == c.dec_layers || xf_ok(m->dec[l + 1].wqkv.w))) f.kz_w2 = 0;      // (the next layer's first norm has to be the XF one)
        f.kz_13 = fin && f.kz_wo && f.kz_w2 && L.w13.w.N == 2 * F && xf_fits(F) ? q4_skinny_mt2_plan(L.w13.w, M) : 0; if (!kz_fits(f.kz_13, 2 * F)) f.kz_13 = 0;
        f.w13 = f.kz_13 ? PF::W13_PLANES : w13_xf ? PF::W13_XF : PF::W13_F32;
        if (f.kz_w2) f.w2 = f.kz_13 ? PF::W2_PLANES_XF : PF::W2_PLANES_ROWS;
        assert(f.valid(l ? &forms[l - 1] : nullptr));
    }
    return forms;
}
static int32_t decoder_prefill_dev(vox_model* m, float* x, int M, vox_cache* kc, int off, int n_seq = 1, long kv_seq_stride = 0) {
    using PF = PrefillLayerForm;
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, KD = KV * hd, W = QD + 2 * KD, F = c.dec_ffn;
    const int seq_rows = n_seq > 1 ? M / n_seq : 0;
    // workspace after the encoder region is reused: [xn | qkv | att | ffn]
    const size_t need = (size_t)M * D + (size_t)M * W + (size_t)M * QD + (size_t)M * F + 1024;
    VOXCHK(ensure(&m->ws, &m->ws_floats, need));
    float* xn = m->ws; float* qkv = xn + (size_t)M * D; float* att = qkv + (size_t)M * W; float* ffn = att + (size_t)M * QD;
    const std::vector<PF> forms = plan_prefill(m, M, n_seq, off, kc->max_seq);
    const DecLayer* L = nullptr; float *kl = nullptr, *vl = nullptr;      // the layer the pieces below work on
    auto rope_kv_store = [&]() -> int32_t {
        HIPCHK(launch_rope(qkv, M, W, QD + KD, hd, off, m->dec_cos, m->dec_sin, s, seq_rows));
        HIPCHK(launch_kv_store(qkv, M, W, QD, KV, hd, off, kl, vl, kc->max_seq * hd, s, seq_rows, kv_seq_stride)); return VOX_OK;
    };
    auto attn_params = [&]() {
        AttnParams ap = prefill_attn_params(c, kc->max_seq, M, n_seq, off); ap.q = qkv; ap.k = kl; ap.v = vl; ap.out = att; ap.kv_seq_stride = kv_seq_stride; return ap;
    };
    // ---- a layer on f32 rows
    auto layer_f32 = [&]() -> int32_t {
        HIPCHK(launch_rms_norm(x, D, M, D, L->attn_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, L->wqkv.w, nullptr, xn, D, M, qkv, W));
        VOXCHK(rope_kv_store());
        HIPCHK(launch_attn_prefill(attn_params(), hd, s, n_seq));
        VOXCHK(q4_linear_dev(cx, L->wo.w, nullptr, att, QD, M, x, D, EPI_RESID, x, D));
        HIPCHK(launch_rms_norm(x, D, M, D, L->ffn_norm, L->ada_mul, c.norm_eps, xn, D, s));    // norm then Ada x*(1+s) (model.rs:382-385)
        VOXCHK(q4_linear_dev(cx, L->w13.w, nullptr, xn, D, M, ffn, F, EPI_SWIGLU));
        VOXCHK(q4_linear_dev(cx, L->w2.w, nullptr, ffn, F, M, x, D, EPI_RESID, x, D)); return VOX_OK;
    };
    // ---- a layer with operators on XF tiles (one sequence); pend = K slices of the previous layer's w2 waiting in the plane buffer.  An operator the planner left on f32 rows runs as above.
    auto gemm_xf = [&](const Q4W& w) { GemmParams p{}; p.w = w; p.xf = reinterpret_cast<const uint4*>(cx->xf_scratch); p.M = M; p.kz_scratch = cx->kz_scratch; p.kz_scratch_bytes = cx->kz_scratch_bytes; return p; };
    auto planes_from_xf = [&](const Q4W& w, int KZ) -> int32_t { HIPCHK(launch_q4_skinny_mt2_planes(gemm_xf(w), KZ, s)); return VOX_OK; };      // this operator over the XF tiles in scratch, into K-slice planes
    auto linear_xf = [&](const Q4W& w, float* out, int out_stride, int epi) -> int32_t {      // ... into f32 rows: launch_q4_gemm picks the kernel, which may split K through the plane buffer
        cx->want_scratch(false, true);
        GemmParams p = gemm_xf(w); p.out = out; p.out_stride = out_stride; HIPCHK(launch_q4_gemm(p, epi, s)); return VOX_OK;
    };
    auto layer_xf = [&](const PF& f, int pend) -> int32_t {
        if (f.qkv == PF::QKV_F32) {      // (pend == 0: PrefillLayerForm::valid)
            HIPCHK(launch_rms_norm(x, D, M, D, L->attn_norm, nullptr, c.norm_eps, xn, D, s));
            VOXCHK(q4_linear_dev(cx, L->wqkv.w, nullptr, xn, D, M, qkv, W));
        } else if (pend) HIPCHK(launch_rms_norm_xf_sumk(x, D, M, D, cx->kz_scratch, pend, L->attn_norm, nullptr, c.norm_eps, cx->xf_scratch, s));      // + the previous layer's w2
        else HIPCHK(launch_rms_norm_xf(x, D, M, D, L->attn_norm, nullptr, c.norm_eps, cx->xf_scratch, s));
        if (f.qkv == PF::QKV_XF) VOXCHK(linear_xf(L->wqkv.w, qkv, W, EPI_STORE));
        if (f.qkv == PF::QKV_PLANES) {
            VOXCHK(planes_from_xf(L->wqkv.w, f.kz_qkv));
            HIPCHK(launch_splitk_finish_rope_kv(cx->kz_scratch, f.kz_qkv, M, W, qkv, W, QD, KV, hd, off, m->dec_cos, m->dec_sin, kl, vl, kc->max_seq * hd, s));
        } else VOXCHK(rope_kv_store());
        AttnParams ap = attn_params();
        if (f.wo == PF::WO_PLANES_XF) { ap.out_xf_tiles = cx->xf_scratch; ap.out_xf_tile_stride = (long)2 * (QD >> 7) * 256 * 8; }
        HIPCHK(launch_attn_prefill(ap, hd, s, n_seq));
        if (f.wo == PF::WO_F32) {
            VOXCHK(q4_linear_dev(cx, L->wo.w, nullptr, att, QD, M, x, D, EPI_RESID, x, D));
            if (f.w13 == PF::W13_F32) HIPCHK(launch_rms_norm(x, D, M, D, L->ffn_norm, L->ada_mul, c.norm_eps, xn, D, s));    // norm then Ada x*(1+s) (model.rs:382-385)
            else HIPCHK(launch_rms_norm_xf(x, D, M, D, L->ffn_norm, L->ada_mul, c.norm_eps, cx->xf_scratch, s));
        } else {
            if (f.wo == PF::WO_PLANES_ROWS) HIPCHK(launch_xf_rows(att, QD, M, QD, cx->xf_scratch, s));
            VOXCHK(planes_from_xf(L->wo.w, f.kz_wo));
            HIPCHK(launch_rms_norm_xf_sumk(x, D, M, D, cx->kz_scratch, f.kz_wo, L->ffn_norm, L->ada_mul, c.norm_eps, cx->xf_scratch, s));      // x += wo(att); norm then Ada x*(1+s) (model.rs:382-385)
        }
        if (f.w13 == PF::W13_F32) VOXCHK(q4_linear_dev(cx, L->w13.w, nullptr, xn, D, M, ffn, F, EPI_SWIGLU));
        if (f.w13 == PF::W13_XF) VOXCHK(linear_xf(L->w13.w, ffn, F, EPI_SWIGLU));
        if (f.w13 == PF::W13_PLANES) {
            VOXCHK(planes_from_xf(L->w13.w, f.kz_13));
            HIPCHK(launch_splitk_finish_swiglu_xf(cx->kz_scratch, f.kz_13, M, 2 * F, nullptr, cx->xf_scratch, s));
        }
        if (f.w2 == PF::W2_F32) return q4_linear_dev(cx, L->w2.w, nullptr, ffn, F, M, x, D, EPI_RESID, x, D);
        if (f.w2 == PF::W2_PLANES_ROWS) HIPCHK(launch_xf_rows(ffn, F, M, F, cx->xf_scratch, s));
        return planes_from_xf(L->w2.w, f.kz_w2);      // summed by the next layer's first norm
    };
    for (int l = 0; l < c.dec_layers; l++) {
        L = &m->dec[l]; kl = kc->k + (size_t)l * kc->layer_stride; vl = kc->v + (size_t)l * kc->layer_stride;
        VOXCHK(forms[l].f32_rows() ? layer_f32() : layer_xf(forms[l], l ? forms[l - 1].kz_w2 : 0));
    }
    if (!forms.empty() && forms.back().kz_w2) HIPCHK(launch_splitk_finish_resid(cx->kz_scratch, forms.back().kz_w2, M, D, x, D, s));      // the last layer's w2
    return VOX_OK;
}

// ---- one decode step on device (Appendix B of SURVEY.md): 4 fused launches per layer -- q|k|v (+ RMSNorm, RoPE, cache write), attention + wo
// (attn_wo_kernel), w1|w3 (+ sum of the wo partials, residual, RMSNorm * Ada, SwiGLU), w2 (+ residual) -- or 5 (separate attention and wo
// launches) for dense checkpoints / other head geometries.  h [D] in place.  position = (pos_ptr ? *pos_ptr : 0) + pos_off.
// May this layer run as four launches?
static bool decode_layer_fuses_attn_wo(const vox_model* m, const DecLayer& L, const AttnParams& ap, const vox_cache* kc) {
    const vox_model_cfg& c = m->cfg; const int D = c.dec_dim;
    return attn_wo_supported(ap, L.wo.w, c.dec_head_dim, kc->max_seq) && L.w13.w.fmt == WFMT_Q4_0 && L.w2.w.fmt == WFMT_Q4_0 /* w2's kernel clears the accumulators */ && L.wo.w.N == D && D % 4 == 0 && L.w13.w.K == 3072 &&
           q4_gemv_default_R(L.w13.w.N, L.w13.w.K, EPI_SWIGLU) == 2;
}

// attn_wo accumulators: every step leaves them cleared (w2 does it); clearing them outright before a run of steps keeps a call that failed half-way through a layer from
// leaking into the next one
static int32_t wo_acc_clear(vox_model* m, hipStream_t s) { if (m->d_wo_acc) HIPCHK(hipMemsetAsync(m->d_wo_acc, 0, (size_t)m->cfg.dec_layers * m->cfg.dec_dim * 8, s)); return VOX_OK; }
// ring (an endless session's step from its wrap on): the cache is a RING of kc->max_seq rows -- the q|k|v GEMV appends at row position % max_seq and reads its RoPE row
// from the session's ring (EPI_ROPE_KV_RING), the per-head ring attention follows, then the wo GEMV: the fused attention + wo launch has no ring form
struct DecRingStep { const float* rope; int mask; };      // the session's decoder RoPE ring [mask + 1][cos hd/2 | sin hd/2]
static int32_t decoder_step_dev(vox_model* m, float* h, vox_cache* kc, const int* pos_ptr, int pos_off, const DecRingStep* ring = nullptr) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, KD = KV * hd, F = c.dec_ffn;
    const size_t lf = kc->layer_stride;
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayer& L = m->dec[l]; float* kl = kc->k + (size_t)l * lf; float* vl = kc->v + (size_t)l * lf;
        GemvParams p{};
        p.w = L.wqkv.w; p.x = h; p.x_stride = D; p.out = m->d_q; p.out_stride = QD; p.gamma = L.attn_norm; p.eps = c.norm_eps;
        p.pos_ptr = pos_ptr; p.pos_off = pos_off; p.rope_cos = m->dec_cos; p.rope_sin = m->dec_sin; p.hd = hd; p.n_q = QD; p.n_k = KD;
        p.kcache = kl; p.vcache = vl; p.cache_head_stride = kc->max_seq * hd;
        if (ring) { p.rope_cos = ring->rope; p.rope_sin = ring->rope + hd / 2; p.rope_mask = ring->mask; }
        {
            HIPCHK(launch_q4_gemv(p, 1, PRO_RMS, ring ? EPI_ROPE_KV_RING : EPI_ROPE_KV, q4_gemv_default_R(p.w.N, p.w.K, EPI_ROPE_KV), s));
            AttnParams ap{}; ap.q = m->d_q; ap.k = kl; ap.v = vl; ap.kv_row_stride = hd; ap.kv_head_stride = kc->max_seq * hd; ap.out = m->d_att;
            ap.n_heads = H; ap.n_kv_heads = KV; ap.offset = pos_off; ap.window = c.dec_window; ap.pos_ptr = pos_ptr; ap.M = 1; ap.spec_rows = kc->max_seq;
            // four launches per layer: attention + wo in one (32-way K split, one partial product per head, combined with int64 fixed-point atomics);
            // w1|w3's prologue adds the sum to the residual and writes the new residual stream (d_h2) for w2's epilogue
            const int R13 = q4_gemv_default_R(L.w13.w.N, L.w13.w.K, EPI_SWIGLU);
            if (!ring && decode_layer_fuses_attn_wo(m, L, ap, kc) && h != m->d_h2) {
                long long* acc = m->d_wo_acc + (size_t)l * D;      // zero on entry: cleared at allocation, and by w2 below after every use
                HIPCHK(launch_attn_wo(ap, L.wo.w, acc, kc->max_seq, s));
                GemvParams f{}; f.w = L.w13.w; f.x = h; f.x_stride = D; f.out = m->d_act; f.out_stride = F; f.gamma = L.ffn_norm; f.mul = L.ada_mul; f.eps = c.norm_eps;
                f.xacc = acc; f.x_out = m->d_h2;
                HIPCHK(launch_q4_gemv(f, 1, PRO_RMS_MUL_SUM, EPI_SWIGLU, R13, s));
                GemvParams d{}; d.w = L.w2.w; d.x = m->d_act; d.x_stride = F; d.out = h; d.out_stride = D; d.resid = m->d_h2; d.resid_stride = D;
                d.zero_acc = acc; d.zero_n = D;                  // w1|w3 has consumed the accumulators: clear them for the next step (no fill node in the graph)
                HIPCHK(launch_q4_gemv(d, 1, PRO_NONE, EPI_RESID, q4_gemv_default_R(d.w.N, d.w.K, EPI_RESID), s));
                continue;
            }
            HIPCHK(ring ? launch_attn_decode_ring(ap, hd, kc->max_seq, s) : launch_attn_decode(ap, hd, kc->max_seq, s));
        }
        GemvParams o{}; o.w = L.wo.w; o.x = m->d_att; o.x_stride = QD; o.out = h; o.out_stride = D; o.resid = h; o.resid_stride = D;
        HIPCHK(launch_q4_gemv(o, 1, PRO_NONE, EPI_RESID, q4_gemv_default_R(o.w.N, o.w.K, EPI_RESID), s));
        GemvParams f{}; f.w = L.w13.w; f.x = h; f.x_stride = D; f.out = m->d_act; f.out_stride = F; f.gamma = L.ffn_norm; f.mul = L.ada_mul; f.eps = c.norm_eps;
        HIPCHK(launch_q4_gemv(f, 1, PRO_RMS_MUL, EPI_SWIGLU, q4_gemv_default_R(f.w.N, f.w.K, EPI_SWIGLU), s));
        GemvParams d{}; d.w = L.w2.w; d.x = m->d_act; d.x_stride = F; d.out = h; d.out_stride = D; d.resid = h; d.resid_stride = D;
        HIPCHK(launch_q4_gemv(d, 1, PRO_NONE, EPI_RESID, q4_gemv_default_R(d.w.N, d.w.K, EPI_RESID), s));
    }
    return VOX_OK;
}

// decode engine: per-CU weight stream (a second copy of the decoder's Q4 bytes in consumption order, built on the GPU from the row planes), granule state, layer table
// the engines' weight stream (shared by the single-stream and the batched engine), packed on the GPU from the row planes at first use.  An allocation failure is not an
// error of the call: the engines are switched off and the launch-based paths serve it.
static int32_t engine_stream_prepare(vox_model* m) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (m->eng_ready || !m->eng_ok) return VOX_OK;
    const size_t sb = eng_stream_bytes(c.dec_layers, c.vocab);
    if (!m->eng_stream) {
        hipError_t e = hipMalloc((void**)&m->eng_stream, sb);
        if (e == hipSuccess) e = hipMalloc((void**)&m->eng_state, eng_state_bytes());
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (m->eng_stream) (void)hipFree(m->eng_stream); if (m->eng_state) (void)hipFree(m->eng_state);
            m->eng_stream = nullptr; m->eng_state = nullptr; m->eng_ok = false; m->eng_on = false; m->engb_ok = false;
            fprintf(stderr, "[voxtral_hip] decode engine: allocating the %.2f GB weight stream failed (%s); the launch-based decode paths are used\n", sb / 1e9, hipGetErrorString(e));
            return VOX_OK;
        }
    }
    HIPCHK(hipMemsetAsync(m->eng_stream, 0, sb, s)); HIPCHK(hipMemsetAsync(m->eng_state, 0, eng_state_bytes(), s));
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayer& L = m->dec[l];
        HIPCHK(launch_eng_pack(L.wqkv.w, 0, l, c.dec_layers, m->eng_stream, c.vocab, s)); HIPCHK(launch_eng_pack(L.wo.w, 1, l, c.dec_layers, m->eng_stream, c.vocab, s));
        HIPCHK(launch_eng_pack(L.w13.w, 2, l, c.dec_layers, m->eng_stream, c.vocab, s)); HIPCHK(launch_eng_pack(L.w2.w, 3, l, c.dec_layers, m->eng_stream, c.vocab, s));
    }
    HIPCHK(launch_eng_pack(m->tok.w, 4, 0, c.dec_layers, m->eng_stream, c.vocab, s));
    m->eng_ready = true;
    return VOX_OK;
}
// batched engine: the stream + one edge-buffer block and layer table per 16-row group
static bool engb_prepare(vox_model* m, int n_grp) {
    if (!m->engb_ok || !m->engb_on || n_grp > 4) return false;
    if (engine_stream_prepare(m) != VOX_OK || !m->eng_ready) return false;
    if (engb_prepare_kernels() != hipSuccess) { (void)hipGetLastError(); m->engb_ok = false; return false; }
    if (!m->eng_wob) {      // wo once more, in the batched engine's XCD-group K split (184 MB for 26 layers)
        const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
        hipError_t e = hipMalloc((void**)&m->eng_wob, engb_wo_stream_bytes(c.dec_layers));
        if (e == hipSuccess) e = hipMemsetAsync(m->eng_wob, 0, engb_wo_stream_bytes(c.dec_layers), s);
        for (int l = 0; l < c.dec_layers && e == hipSuccess; l++) e = launch_eng_pack(m->dec[l].wo.w, 5, l, c.dec_layers, m->eng_wob, c.vocab, s);
        if (e != hipSuccess) { (void)hipGetLastError(); if (m->eng_wob) { (void)hipFree(m->eng_wob); m->eng_wob = nullptr; } m->engb_ok = false; return false; }
    }
    for (int gi = 0; gi < n_grp; gi++) {
        if (m->engb_state[gi]) continue;
        hipError_t e = hipMalloc((void**)&m->engb_state[gi], engb_state_bytes());
        if (e == hipSuccess) e = hipMalloc((void**)&m->engb_tab[gi], sizeof(EngLayerTab) * 32);
        if (e == hipSuccess) e = engb_state_init(m->engb_state[gi], m->ctx->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); if (m->engb_state[gi]) { (void)hipFree(m->engb_state[gi]); m->engb_state[gi] = nullptr; } return false; }
    }
    return true;
}
// a hand-off timeout inside the single-stream engine (its error word was read as non-zero): count the strike, re-arm the engine's state for the next launch, drop the
// captured decode graphs; three strikes switch the engine off for the life of the model.  What each caller re-runs, and what it tells its user, is the caller's.
static int32_t engine_strike(vox_model* m) {
    m->eng_strikes++;
    HIPCHK(hipMemsetAsync(m->eng_state, 0, eng_state_bytes(), m->ctx->stream)); m->eng_launches = 0; graphs_destroy(m);
    if (m->eng_strikes >= 3) { m->eng_ok = false; m->eng_on = false; }
    return VOX_OK;
}
// ---- the single-stream engine's host side, shared by its clients (transcribe_dev, the piecewise decoder surface, vox_stream, vox_bench_decode_gemv).  Which path a step
// took stays visible at every call site: the clients count steps by path, and each keeps its own recovery from a hand-off timeout.
static const int ENGINE_MAX_ROWS = 1024;      // long caches keep the per-operator path (attention scores live in LDS)
// the engines' view of the decoder layers over K / V planes [layer][..] that start at k / v: out[l] for every layer (group_off: a 16-row group's slice inside each layer)
static void dec_layer_tab(const vox_model* m, float* k, float* v, size_t layer_stride, size_t group_off, EngLayerTab* out) {
    for (size_t l = 0, o = group_off; l < (size_t)m->cfg.dec_layers; l++, o += layer_stride) out[l] = EngLayerTab{m->dec[l].attn_norm, m->dec[l].ffn_norm, m->dec[l].ada_mul, k + o, v + o};
}
// may the engine serve steps against this cache?  (suspended: a client is re-running steps on the per-operator path after a hand-off timeout)
static bool engine_serves(const vox_model* m, const vox_cache* kc) { return m->eng_ok && m->eng_on && !m->eng_suspended && kc && kc->max_seq <= ENGINE_MAX_ROWS; }
// the binding's table for `kc`, on its way to the device (the host copy lives in the binding: nothing to wait for)
static hipError_t engine_tab_enqueue(vox_model* m, EngBinding& b, const vox_cache* kc) {
    b.host.resize(m->cfg.dec_layers); dec_layer_tab(m, kc->k, kc->v, kc->layer_stride, 0, b.host.data());
    const hipError_t e = hipMemcpyAsync(b.tab, b.host.data(), sizeof(EngLayerTab) * b.host.size(), hipMemcpyHostToDevice, m->ctx->stream);
    b.cache = e == hipSuccess ? kc : nullptr; b.gen = kc->gen; return e;
}
// allocates whatever the binding still lacks (bytes: where a client that reports its footprint counts the device buffers)
static hipError_t binding_alloc(const vox_model* m, EngBinding& b, uint64_t* bytes = nullptr) {
    hipError_t e = hipSuccess; auto A = [&](void** q, size_t n) { if (e == hipSuccess && !*q && (e = hipMalloc(q, n)) == hipSuccess && bytes) *bytes += n; };
    A((void**)&b.tab, sizeof(EngLayerTab) * std::max(m->cfg.dec_layers, 32)); A((void**)&b.part_val, 256 * 4); A((void**)&b.part_idx, 256 * 4);
    if (e == hipSuccess && !b.err_word) { e = hipHostMalloc((void**)&b.err_word, 8, hipHostMallocDefault); if (e == hipSuccess) b.err_word[0] = b.err_word[1] = 0u; else b.err_word = nullptr; }
    return e;
}
// May this client launch the engine against `kc` now?  Packs the weight stream at first use, allocates what the binding lacks, and rebuilds the layer table only for a
// cache (or a generation of it: a freed cache's address may be handed out again) the binding does not hold -- a step on a bound cache copies and synchronises nothing.
// A failure in here is not an error of the call: the per-operator launches serve it.
static bool engine_bind(vox_model* m, EngBinding& b, const vox_cache* kc) {
    if (!engine_serves(m, kc) || engine_stream_prepare(m) != VOX_OK || !m->eng_ready) return false;
    hipError_t e = binding_alloc(m, b);
    if (e == hipSuccess && (b.cache != kc || b.gen != kc->gen)) { e = engine_tab_enqueue(m, b, kc); if (e == hipSuccess) e = hipStreamSynchronize(m->ctx->stream); }
    if (e != hipSuccess) { (void)hipGetLastError(); b.cache = nullptr; }
    return e == hipSuccess;
}
// one launch's parameters: the client's table, partials and cache; input row, position = *pos_ptr + pos_off, optional f32 logits
static EngParams engine_params(vox_model* m, const EngBinding& b, const vox_cache* kc, const float* h_in, const int* pos_ptr, int pos_off, float* logits_out) {
    const vox_model_cfg& c = m->cfg;
    EngParams ep{}; ep.stream = m->eng_stream; ep.cu_stride = eng_stream_bytes(c.dec_layers, c.vocab) / 256; ep.layers = b.tab; ep.n_layers = c.dec_layers; ep.h_in = h_in; ep.final_norm = m->dec_norm;
    ep.pos_ptr = pos_ptr; ep.pos_off = pos_off; ep.rope_cos = m->dec_cos; ep.rope_sin = m->dec_sin; ep.max_seq = kc->max_seq; ep.window = c.dec_window; ep.eps = c.norm_eps;
    eng_state_carve(m->eng_state, &ep); ep.part_val = b.part_val; ep.part_idx = b.part_idx; ep.logits_out = logits_out; ep.vocab = c.vocab; ep.tl = nullptr; ep.tl_layer = -1;
    ep.flags = m->eng_flags; ep.pace_ticks = (m->eng_flags & 512) ? 0 : m->eng_pace; ep.ag_delay_ticks = (m->eng_flags & 512) ? m->eng_pace : 0;
    return ep;
}
// before n launches are enqueued: tags = (launch serial + 1) * 64 + layer + 1 are 32-bit -- restart the serial long before they wrap (never inside a captured graph)
static int32_t engine_take_serials(vox_model* m, unsigned long long n, hipStream_t s) {
    if (m->eng_launches + n > (1ull << 25)) { HIPCHK(hipMemsetAsync(m->eng_state, 0, eng_state_bytes(), s)); m->eng_launches = 0; }
    m->eng_launches += n; return VOX_OK;
}
// the engine's error word (first failure code of the launches so far, 0 = ok) on its way to a host word: lands with the next synchronisation of s
static int32_t engine_err_enqueue(vox_model* m, unsigned* dst, hipStream_t s) {
    EngParams ep{}; eng_state_carve(m->eng_state, &ep); HIPCHK(hipMemcpyAsync(dst, ep.err, 8, hipMemcpyDeviceToHost, s)); return VOX_OK;
}
// how every client names a non-zero error word e (strikes 0: a measurement launch, no strike is counted)
static std::string engine_timeout_text(unsigned e, int strikes) {
    char b[96]; const int n = snprintf(b, sizeof b, "hand-off timeout (code %u, workgroup %u)", e & 0xff, (e >> 8) & 0xff);
    if (strikes > 0) snprintf(b + n, sizeof b - n, ", strike %d of 3", strikes);
    return b;
}
// while it lives, the engine serves nobody: steps a client runs again after a hand-off timeout take the per-operator launches.  Restores what it found (re-runs nest).
struct EngSuspend { vox_model* m; bool was; explicit EngSuspend(vox_model* m_) : m(m_), was(m_->eng_suspended) { m->eng_suspended = true; } ~EngSuspend() { m->eng_suspended = was; } };

extern "C" int32_t vox_model_set_decode_engine(vox_model* m, int32_t on, int32_t* active) {
    ARGCHK(m, "null argument"); VOXCHK(ctx_bind(m->ctx));
    const bool want = on != 0 && m->eng_ok;
    if (want != m->eng_on) { HIPCHK(hipStreamSynchronize(m->ctx->stream)); graphs_destroy(m); m->eng_on = want; }      // the captured decode graph holds the other path's launches
    if (active) *active = m->eng_on ? 1 : 0;
    return VOX_OK;
}

extern "C" int32_t vox_model_set_batch_engine(vox_model* m, int32_t on, int32_t* active, uint64_t* launches) {
    ARGCHK(m, "null argument");
    if (on >= 0) m->engb_on = on != 0;
    if (active) *active = m->engb_ok && m->engb_on ? 1 : 0;
    if (launches) *launches = m->engb_launches;
    return VOX_OK;
}

// final RMSNorm + tied lm_head (Q4) + argmax partials (gguf/model.rs:676,680-691,922-923); logits_out optional [vocab]
static int32_t lm_head_argmax_dev(vox_model* m, const float* h, float* logits_out) {
    const vox_model_cfg& c = m->cfg;
    ARGCHK(c.dec_dim <= 4096, "lm_head GEMV is instantiated for dec_dim <= 4096 (got %d)", c.dec_dim);
    GemvParams p{}; p.w = m->tok.w; p.x = h; p.x_stride = c.dec_dim; p.out = logits_out; p.out_stride = c.vocab; p.gamma = m->dec_norm; p.eps = c.norm_eps;
    p.part_val = m->d_part_val; p.part_idx = m->d_part_idx;
    if (m->tok.w.fmt == WFMT_Q4_0) m->n_parts = q4_gemv_grid_k(c.vocab, c.dec_dim, m->argmax_R, EPI_ARGMAX);   // partials = workgroups of THIS launch (<= the allocated count)
    HIPCHK(launch_q4_gemv(p, 1, PRO_RMS, EPI_ARGMAX, m->argmax_R, m->ctx->stream));
    return VOX_OK;
}

static int32_t ensure_decode_state(vox_model* m, int S) {
    if (!m->cache || m->cache->max_seq < S) {
        int cap = std::max(S, 256); cap = std::min((cap + 255) / 256 * 256, m->dec_rope_len);
        ARGCHK(S <= cap, "sequence of %d decoder positions exceeds the RoPE table (%d)", S, m->dec_rope_len);
        if (m->cache) { HIPCHK(hipStreamSynchronize(m->ctx->stream)); cache_release(m->cache); m->eng_offline.cache = nullptr; }
        graphs_destroy(m);
        VOXCHK(cache_alloc(m, cap, &m->cache));
    }
    // token buffer: allocated ONCE for the longest admissible sequence (S <= dec_rope_len) -- the captured decode graph bakes this
    // pointer into argmax_embed_kernel, so it must never move while a graph is alive
    if (!m->d_tokens) { m->tokens_cap = m->dec_rope_len + 2; HIPCHK(hipMalloc((void**)&m->d_tokens, (size_t)m->tokens_cap * 4)); }
    ARGCHK(S + 2 <= m->tokens_cap, "sequence of %d decoder positions exceeds the token buffer", S);
    return VOX_OK;
}

// ---- prefix state (struct PrefixState): what the silent left pad of vox_transcribe_audio makes identical for every utterance
// Bounds from the pad configuration.  Mel frame f reads padded samples [160 f - 200, 160 f + 200) (reflected at the start: still inside the pad), so frames 0 .. Fc =
// (left - 200) / 160 are the constant floor whatever follows; conv-stem row s reads frames 4 s - 3 .. 4 s + 3 (two k3 s2 p1 convolutions), so rows 0 .. (Fc - 3) / 4 are
// constant; the encoder attention is causal and RoPE starts at 0, so these rows stay constant through the layers.  RC = that row count rounded DOWN to a multiple of the
// reshape factor (the adapter's [rows / R][R D] view of the live rows stays aligned); the decoder part covers positions 0 .. 36 = the prefix tokens whose successor is
// also a prefix token, and is used only when the encoder part reaches that far (one ordinary step at position 37 then replaces the whole prefill).
namespace vox_host {
void prefix_release(vox_model* m) {
    PrefixState& p = m->pfx;
    for (float** q : {&p.enc_kv, &p.audio, &p.dec_k, &p.dec_v}) { if (*q) (void)hipFree(*q); *q = nullptr; }
    p.enc_built = p.dec_built = false; p.enc_bytes = p.dec_bytes = 0; p.t_embed.clear();
}
}  // namespace vox_host
static void prefix_bounds(const vox_model* m, int* RC, int* PC) {
    const vox_model_cfg& c = m->cfg; *RC = 0; *PC = 0;
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    const long left = (long)pad_left(&pc), R = c.reshape_factor;
    if (left < 200 || R < 1 || c.n_mels != 128 || (c.enc_head_dim != 64 && c.enc_head_dim != 128) || m->enc.empty() || m->dec.empty()) return;
    const long Fc = (left - 200) / 160, rows = Fc >= 3 ? (Fc - 3) / 4 + 1 : 0;
    const long pcn = VOX_PREFIX_TOKENS - 1;
    if (rows / R < pcn || pcn * R + 4 > m->enc_rope_len) return;
    *PC = (int)pcn; *RC = (int)(pcn * R);
}
static bool prefix_active(const vox_model* m) { int rc, pc; prefix_bounds(m, &rc, &pc); return m->pfx.on && rc > 0; }
// the decoder's fixed prefix on its way into a token buffer: the one upload every caller uses
static hipError_t prefix_tokens_enqueue(int* d_tokens, hipStream_t s) { return hipMemcpyAsync(d_tokens, PREFIX_TOKENS.t, sizeof PREFIX_TOKENS.t, hipMemcpyHostToDevice, s); }
// The prefill half of seeding a decode (seed_clip; prefix_build runs it once per model over its own adapter rows): inputs = audio[:rows] + embed(prefix tokens, already
// in d_tokens) into the model-owned d_prefix (no hipMalloc / hipFree in the timed path), prefilled into the model's cache from row 0 (gguf/model.rs:896-915)
static int32_t prefill_prefix_rows(vox_model* m, const float* audio, int rows) {
    const vox_model_cfg& c = m->cfg;
    if (!m->d_prefix) HIPCHK(hipMalloc((void**)&m->d_prefix, (size_t)VOX_PREFIX_TOKENS * c.dec_dim * 4));
    HIPCHK(launch_embed(m->tok.w, m->d_tokens, rows, audio, c.dec_dim, nullptr, 0, 0, m->d_prefix, m->ctx->stream));
    m->cache->len = 0;
    return decoder_prefill_dev(m, m->d_prefix, rows, m->cache, 0);
}
static int32_t prefix_build(vox_model* m, const float* t_embed) {
    PrefixState& p = m->pfx; const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    int RC, PC; prefix_bounds(m, &RC, &PC);
    if (!p.on || RC <= 0) return VOX_OK;
    if (p.enc_built && p.dec_built && p.t_embed.size() == (size_t)c.dec_dim && !std::memcmp(p.t_embed.data(), t_embed, (size_t)c.dec_dim * 4)) return VOX_OK;
    const int QD = c.enc_heads * c.enc_head_dim, hd = c.dec_head_dim, KV = c.dec_kv_heads;
    p.RC = RC; p.PC = PC;
    // device memory for the state; a failed allocation is not an error of the call: the model goes back to the full computation (as the decode engine does without its stream)
    const size_t rows_bytes = (size_t)PC * hd * 4, n_rows = (size_t)c.dec_layers * KV;
    {
        hipError_t e = hipSuccess;
        auto A = [&](float** q, size_t n) { if (e == hipSuccess && !*q) e = hipMalloc((void**)q, n); };
        A(&p.enc_kv, (size_t)c.enc_layers * RC * 2 * QD * 4); A(&p.audio, (size_t)PC * c.dec_dim * 4); A(&p.dec_k, rows_bytes * n_rows); A(&p.dec_v, rows_bytes * n_rows);
        if (e != hipSuccess) {
            (void)hipGetLastError(); prefix_release(m); p.on = false;
            fprintf(stderr, "[voxtral_hip] prefix state: allocating %.1f MB failed (%s); every call runs the full computation\n",
                    ((double)c.enc_layers * RC * 2 * QD * 4 + 2.0 * rows_bytes * n_rows) / 1e6, hipGetErrorString(e));
            return VOX_OK;
        }
    }
    if (!p.enc_built) {
        // the encoder over a silent mel long enough that rows 0 .. RC-1 see nothing but it (RC + 4 rows), made by the mel kernel itself from an all-zero padded signal
        const int Tb = 4 * (RC + 4);
        p.enc_bytes = (uint64_t)c.enc_layers * RC * 2 * QD * 4 + (uint64_t)PC * c.dec_dim * 4;
        MelTables t; VOXCHK(ctx_mel_tables(cx, &t));
        DevBuf mel; HIPCHK(mel.alloc((size_t)c.n_mels * Tb * 4));
        HIPCHK(launch_mel(nullptr, 0, (long)Tb * 160, 0, nullptr, t, mel.as<float>(), Tb, 1, s));
        int S4 = 0; p.capture = p.enc_kv; p.capture_rows = RC;
        const int32_t r = encode_dev(m, mel.as<float>(), Tb, &S4);
        p.capture = nullptr; p.capture_rows = 0;
        VOXCHK(r); ARGCHK(S4 >= PC, "internal: prefix build gave %d audio rows", S4);
        HIPCHK(hipMemcpyAsync(p.audio, m->d_audio, (size_t)PC * c.dec_dim * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));      // (mel is freed at the end of this block)
        p.enc_built = true;
    }
    // the decoder's cache rows 0 .. PC-1: the ordinary prefill over the first PC prefix tokens (rows of a causal prefill do not depend on the rows behind them)
    VOXCHK(vox_model_set_t_embed(m, t_embed));
    VOXCHK(ensure_decode_state(m, VOX_PREFIX_TOKENS));
    p.dec_bytes = 2 * (uint64_t)rows_bytes * n_rows;
    HIPCHK(prefix_tokens_enqueue(m->d_tokens, s));
    VOXCHK(prefill_prefix_rows(m, p.audio, PC));
    const size_t pitch = (size_t)m->cache->max_seq * hd * 4;      // cache: [layer][kv head][max_seq][hd], layers back to back
    ARGCHK(m->cache->layer_stride == (size_t)KV * m->cache->max_seq * hd, "internal: cache layout");
    HIPCHK(hipMemcpy2DAsync(p.dec_k, rows_bytes, m->cache->k, pitch, rows_bytes, n_rows, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpy2DAsync(p.dec_v, rows_bytes, m->cache->v, pitch, rows_bytes, n_rows, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    p.t_embed.assign(t_embed, t_embed + c.dec_dim); p.dec_built = true;      // (after vox_model_set_t_embed, which clears the flag when t_embed changes)
    return VOX_OK;
}
// decoder positions 0 .. PC-1 of the prefix state into a cache: K / V rows of every (layer, kv head) plane, the cache then stands at PC
static int32_t prefix_rows_into(vox_model* m, vox_cache* kc, hipStream_t s) {
    const vox_model_cfg& c = m->cfg; const PrefixState& P = m->pfx;
    const size_t rows_bytes = (size_t)P.PC * c.dec_head_dim * 4, n_rows = (size_t)c.dec_layers * c.dec_kv_heads, pitch = (size_t)kc->max_seq * c.dec_head_dim * 4;
    const size_t plane = (size_t)c.dec_kv_heads * kc->max_seq * c.dec_head_dim, src_layer = (size_t)c.dec_kv_heads * P.PC * c.dec_head_dim;
    if (kc->layer_stride == plane) {      // the layers back to back: one copy per tensor
        HIPCHK(hipMemcpy2DAsync(kc->k, pitch, P.dec_k, rows_bytes, rows_bytes, n_rows, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(kc->v, pitch, P.dec_v, rows_bytes, rows_bytes, n_rows, hipMemcpyDeviceToDevice, s));
    } else for (int l = 0; l < c.dec_layers; l++) {      // one sequence's slice of a slab (a stream group's member)
        HIPCHK(hipMemcpy2DAsync(kc->k + (size_t)l * kc->layer_stride, pitch, P.dec_k + (size_t)l * src_layer, rows_bytes, rows_bytes, c.dec_kv_heads, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(kc->v + (size_t)l * kc->layer_stride, pitch, P.dec_v + (size_t)l * src_layer, rows_bytes, rows_bytes, c.dec_kv_heads, hipMemcpyDeviceToDevice, s));
    }
    kc->len = P.PC; return VOX_OK;
}
// Does THIS call run on the prefix?  Only a clip that decodes at least one position behind the prefix tokens (then at least one live adapter row exists).
static bool prefix_usable(const vox_model* m, int T) {
    const PrefixState& p = m->pfx; const vox_model_cfg& c = m->cfg;
    if (!p.on || !p.enc_built || !p.dec_built || p.RC <= 0 || knob_str("VOX_ATTN_F32")) return false;
    const int S = enc_rows(T);
    return S / c.reshape_factor > VOX_PREFIX_TOKENS && S <= m->enc_rope_len;
}
extern "C" int32_t vox_model_set_prefix_cache(vox_model* m, int32_t on, int32_t* active) {
    ARGCHK(m, "null argument"); VOXCHK(ctx_bind(m->ctx));
    if (on >= 0) {
        m->pfx.on = on != 0;
        if (!m->pfx.on) { HIPCHK(hipStreamSynchronize(m->ctx->stream)); prefix_release(m); }
        else if (m->t_embed_set) { std::vector<float> te = m->t_embed_host; VOXCHK(prefix_build(m, te.data())); }      // (before the first utterance the build waits for its t_embed)
    }
    if (active) *active = prefix_active(m) ? 1 : 0;
    return VOX_OK;
}
extern "C" int32_t vox_model_prefix_info(const vox_model* m, int32_t out[4]) {
    ARGCHK(m && out, "null argument");
    int rc, pc; prefix_bounds(m, &rc, &pc);
    const uint64_t b = (m->pfx.enc_kv ? m->pfx.enc_bytes : 0) + (m->pfx.dec_k ? m->pfx.dec_bytes : 0);
    out[0] = m->pfx.enc_built && m->pfx.dec_built ? 1 : 0; out[1] = rc; out[2] = pc; out[3] = (int32_t)std::min<uint64_t>(b, 0x7fffffff);
    return VOX_OK;
}

// one full sync-free decode step, in the launch form `how` (StepLaunch). On entry d_h holds the step's input embedding (audio[cur] + embed(token[cur])):
// 26 layers -> final norm + lm_head (argmax partials) -> fused tail: token[cur+1], cur++, next step's d_h.
// eng: engine_bind(m, m->eng_offline, m->cache) said yes for this utterance (EngineAlone and EngineArgmaxFirst exist only then).
static int32_t decode_step_enqueue(vox_model* m, float* logits_out, bool eng, StepLaunch how = StepLaunch::StepAndArgmax) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (eng) {      // one launch: 26 layers + final norm + lm_head + per-CU argmax partials
        EngParams ep = engine_params(m, m->eng_offline, m->cache, m->d_h, m->d_pos, 0, logits_out);
        if (how == StepLaunch::EngineArgmaxFirst) {      // the launch forms its own input: argmax of the previous launch's partials, token -> d_tokens, embedding + audio row (vox_engine.hip comm_next_input)
            ep.flags |= 65536; ep.h_in = nullptr; ep.tokens = m->d_tokens; ep.pos_rw = m->d_pos; ep.tok_qs = m->tok.w.qs; ep.tok_sc = m->tok.w.sc; ep.tok_nb = m->tok.w.nb; ep.audio = m->d_audio;
        }
        HIPCHK(launch_decode_engine(ep, s));
        if (how == StepLaunch::StepAndArgmax) HIPCHK(launch_argmax_embed(m->d_part_val, m->d_part_idx, 256, m->d_tokens, m->d_pos, m->tok.w, m->d_audio, c.dec_dim, m->d_h, s));
        return VOX_OK;
    }
    VOXCHK(decoder_step_dev(m, m->d_h, m->cache, m->d_pos, 0));
    VOXCHK(lm_head_argmax_dev(m, m->d_h, logits_out));
    HIPCHK(launch_argmax_embed(m->d_part_val, m->d_part_idx, m->n_parts, m->d_tokens, m->d_pos, m->tok.w, m->d_audio, c.dec_dim, m->d_h, s));
    return VOX_OK;
}

// ---- the single-clip driver (vox_transcribe_streaming, vox_transcribe_audio): transcribe_dev = encode, plan_clip, clip_attempt (seed_clip, run_decode_steps, copy-out,
// one synchronisation, a verdict on the engine), the re-run policy after a hand-off timeout.
// What a clip of S decoder positions asks of the decoder.  The reference: fewer than 38 positions give no ids (gguf/model.rs:887-889); the 38-token prefix is prefilled, the
// argmax of its last row is the first id, tokens[38] (922-926); every pos in 39 .. S-1 is one step and one more id (938).  Here the ids are tokens[38 .. 38 + n_ids): the cache
// is seeded with rows 0 .. first_pos - 1, then `steps` decode steps run from first_pos on, and first_pos + steps = max(S - 1, 38) rows stand in the cache afterwards.
//   full form    first_pos = 38 (prefilled; tokens[38] from the prefill's lm_head), steps = max(S - 39, 0), n_ids = 1 + steps
//   on prefix    first_pos = PC = 37 (rows copied from the model's prefix state; S > 38 there: prefix_usable), steps = S - 38 = n_ids: tokens[38] is the first step's
struct ClipPlan { int S = 0, n_ids = 0, first_pos = 0, steps = 0; bool on_prefix = false, want_logits = false; };
static ClipPlan plan_clip(int S, bool on_prefix, int PC, bool want_logits) {
    ClipPlan p; p.S = S; p.on_prefix = on_prefix; p.want_logits = want_logits;
    if (S < VOX_PREFIX_TOKENS) return p;      // n_ids == 0: nothing to decode
    p.n_ids = std::max(S - VOX_PREFIX_TOKENS, 1);
    p.first_pos = on_prefix ? PC : VOX_PREFIX_TOKENS;
    p.steps = on_prefix ? S - PC - 1 : std::max(S - VOX_PREFIX_TOKENS - 1, 0);
    return p;
}

// Leaves the model ready for the plan's first decode step: prefix tokens, cache rows 0 .. first_pos - 1, d_pos = first_pos; the full form also tokens[38] and (logits
// tap) logits row 0.  Opens the roctx stage "prefill" behind the token upload.
static int32_t seed_clip(vox_model* m, const ClipPlan& plan, DevBuf& dlog, RoctxStage& stage) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    HIPCHK(prefix_tokens_enqueue(m->d_tokens, s));
    m->cache->len = 0;
    stage.begin("prefill");
    if (plan.on_prefix) {
        // Positions 0 .. PC-1 (= 36) are the model's: their K / V rows are copied into the cache (every call: the cache may have been re-allocated, and a decode overwrites
        // nothing below PC but a batch call may), and position PC = 37 -- the last prefix token, the first one whose output is kept -- runs as the first ordinary decode
        // step: no prefill, no separate lm_head; tokens[38] comes out of the same argmax chain as every later token.
        VOXCHK(prefix_rows_into(m, m->cache, s));
    } else {
        VOXCHK(prefill_prefix_rows(m, m->d_audio, plan.first_pos));
        m->cache->len = plan.first_pos;
        // lm_head on the last prefix row only (the reference computes all 38 and keeps the last, model.rs:916-923)
        if (plan.want_logits) HIPCHK(dlog.alloc((size_t)plan.n_ids * c.vocab * 4));
        VOXCHK(lm_head_argmax_dev(m, m->d_prefix + (size_t)(plan.first_pos - 1) * c.dec_dim, dlog.as<float>()));
    }
    HIPCHK(hipMemcpyAsync(m->d_pos, &plan.first_pos, 4, hipMemcpyHostToDevice, s));      // (the plan outlives the attempt's synchronisation)
    if (!plan.on_prefix) HIPCHK(launch_argmax_final(m->d_part_val, m->d_part_idx, m->n_parts, m->d_tokens, m->d_pos, 0, 0, s));   // tokens[38]
    return VOX_OK;
}

namespace vox_host {
void graphs_destroy(vox_model* m) {
    DecodeGraphs& g = m->graphs;
    for (int i = 0; i < 2; i++) {
        if (g.exec[i]) { (void)hipGraphExecDestroy(g.exec[i]); g.exec[i] = nullptr; }
        if (g.graph[i]) { (void)hipGraphDestroy(g.graph[i]); g.graph[i] = nullptr; }
    }
}
}  // namespace vox_host
// the decode graphs for `key`: whatever was captured under another key is dropped first
static DecodeGraphs& graphs_for(vox_model* m, const DecodeGraphs::Key& key) {
    const DecodeGraphs::Key& k = m->graphs.key;
    if (k.cache != key.cache || k.audio != key.audio || k.unroll != key.unroll || k.launch != key.launch) { graphs_destroy(m); m->graphs.key = key; }
    return m->graphs;
}
// captures n_steps steps of the graphs' launch form as graph `which`; a failed enqueue still ends the capture, the first error is the one reported
static int32_t graph_capture(vox_model* m, int which, int n_steps, bool eng) {
    DecodeGraphs& g = m->graphs; hipStream_t s = m->ctx->stream;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int32_t r = VOX_OK;
    for (int i = 0; i < n_steps && r == VOX_OK; i++) r = decode_step_enqueue(m, nullptr, eng, g.key.launch);
    hipError_t ce = hipStreamEndCapture(s, &g.graph[which]);
    if (r != VOX_OK) return r;
    HIPCHK(ce);
    HIPCHK(hipGraphInstantiate(&g.exec[which], g.graph[which], nullptr, nullptr, 0));
    return VOX_OK;
}
// steps per replayed graph.  VOX_DECODE_UNROLL=U (measurement knob) builds a U-step graph for the bulk of the steps next to the one-step graph; measured in round 2
// (profiles/r02_decode_knobs.txt): no gain on the per-operator path -- graph boundaries are not where the time goes.  With the engine's one or two launches per step
// the boundaries show: 8 steps per graph by default there.
static int decode_unroll(bool eng) { const char* e = knob_str("VOX_DECODE_UNROLL"); return e && atoi(e) >= 1 && atoi(e) <= 32 ? atoi(e) : eng ? 8 : 1; }
// the one-step graph exists, `done` of `steps` steps are enqueued: the rest as replays, U-step graphs first (built only for long enough utterances), then single steps
static int32_t replay_rest(vox_model* m, bool eng, int done, int steps) {
    DecodeGraphs& g = m->graphs; hipStream_t s = m->ctx->stream; const int U = g.key.unroll;
    if (U > 1 && !g.exec[1] && steps - done >= 2 * U) VOXCHK(graph_capture(m, 1, U, eng));
    while (U > 1 && g.exec[1] && steps - done >= U) { HIPCHK(hipGraphLaunch(g.exec[1], s)); done += U; m->timings.graph_replays += U; }
    while (done < steps) { HIPCHK(hipGraphLaunch(g.exec[0], s)); done++; m->timings.graph_replays++; }
    return VOX_OK;
}
// The three step drivers.  (1) eager, a logits row per step (the logits tap): row i + 1 of d_logits_all is the output of step i
static int32_t steps_eager_logits(vox_model* m, const ClipPlan& plan, bool eng, float* d_logits_all) {
    int32_t r = VOX_OK; for (int i = 0; i < plan.steps && r == VOX_OK; i++) r = decode_step_enqueue(m, d_logits_all + (size_t)(i + 1) * m->cfg.vocab, eng);
    return r;
}
// (2) graph replay of two-launch steps: the per-operator launches, or the engine under VOX_ENGINE_ARGMAX_IN=0 (measurement knob)
static int32_t steps_replayed(vox_model* m, const ClipPlan& plan, bool eng) {
    const DecodeGraphs& g = graphs_for(m, {m->cache, m->d_audio, decode_unroll(eng), StepLaunch::StepAndArgmax});
    int done = 0;
    if (!g.exec[0]) {
        VOXCHK(decode_step_enqueue(m, nullptr, eng)); done = 1;      // eager first step (also warms function attributes)
        HIPCHK(hipStreamSynchronize(m->ctx->stream));
        VOXCHK(graph_capture(m, 0, 1, eng));
    }
    return replay_rest(m, eng, done, plan.steps);
}
// (3) the engine's chained form: a step is ONE launch.  The utterance's first step runs eagerly as a plain launch (its input is in d_h), the replayed launches take
// their input from the previous launch's argmax partials themselves, and one argmax_final behind the last step writes the last token.
static int32_t steps_chained(vox_model* m, const ClipPlan& plan) {
    hipStream_t s = m->ctx->stream;
    const DecodeGraphs& g = graphs_for(m, {m->cache, m->d_audio, decode_unroll(true), StepLaunch::EngineArgmaxFirst});
    VOXCHK(decode_step_enqueue(m, nullptr, true, StepLaunch::EngineAlone));
    if (!g.exec[0]) { HIPCHK(hipStreamSynchronize(s)); VOXCHK(graph_capture(m, 0, 1, true)); }
    VOXCHK(replay_rest(m, true, 1, plan.steps));
    HIPCHK(launch_argmax_final(m->d_part_val, m->d_part_idx, 256, m->d_tokens, m->d_pos, 1, 1, s));      // the last step's token
    return VOX_OK;
}
// the plan's decode steps behind seed_clip: the first step's input, then one of the three drivers
static int32_t run_decode_steps(vox_model* m, const ClipPlan& plan, bool eng, float* d_logits_all) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (plan.steps <= 0) return VOX_OK;
    VOXCHK(wo_acc_clear(m, s));      // once per utterance
    HIPCHK(launch_embed(m->tok.w, m->d_tokens, 1, m->d_audio, c.dec_dim, m->d_pos, 0, 0, m->d_h, s));   // input of the first decode step (audio[38] exists iff S >= 39; on the prefix: audio[37] + embed(PAD))
    if (plan.want_logits) return steps_eager_logits(m, plan, eng, d_logits_all);
    const char* k = knob_str("VOX_ENGINE_ARGMAX_IN");
    return eng && !(k && k[0] == '0') ? steps_chained(m, plan) : steps_replayed(m, plan, eng);
}

// One attempt at the plan on the model's own cache: decode state, engine binding and launch serials, seed_clip, run_decode_steps, ids (and logits) on their way to the
// caller, the engine's error word behind them, ONE synchronisation.  *eng_timed_out: a bounded hand-off wait expired inside the engine -- the ids of this attempt are
// not trustworthy (m->eng_offline.err_word holds the code); what happens then is the caller's.
// rec: also a record per id from the kept logits rows (launch_records_rows, once over all rows), into the caller's host arrays behind the same synchronisation.
struct ClipRecords { vox_token_score* scores; vox_token_alts* alts; int k; };      // what a scored call asked for: host arrays (either may be null) and k
static int32_t clip_attempt(vox_model* m, const ClipPlan& plan, int32_t* out_ids, float* logits_host, const ClipRecords* rec, bool* eng_timed_out) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    *eng_timed_out = false;
    VOXCHK(ensure_decode_state(m, plan.S));
    const bool eng = engine_bind(m, m->eng_offline, m->cache); if (eng) VOXCHK(engine_take_serials(m, (unsigned long long)plan.S + 8, s));
    DevBuf dlog; RoctxStage stage;      // dlog: the logits tap's rows, allocated by seed_clip (null without the tap)
    VOXCHK(seed_clip(m, plan, dlog, stage));
    float* const d_logits_all = dlog.as<float>();
    stage.begin("decode");
    VOXCHK(run_decode_steps(m, plan, eng, d_logits_all));
    HIPCHK(hipMemcpyAsync(out_ids, m->d_tokens + VOX_PREFIX_TOKENS, (size_t)plan.n_ids * 4, hipMemcpyDeviceToHost, s));
    if (logits_host) HIPCHK(hipMemcpyAsync(logits_host, d_logits_all, (size_t)plan.n_ids * c.vocab * 4, hipMemcpyDeviceToHost, s));
    DevBuf dsc, dal;
    if (rec) {
        if (rec->scores) HIPCHK(dsc.alloc((size_t)plan.n_ids * sizeof(TokenScore)));
        if (rec->alts) HIPCHK(dal.alloc((size_t)plan.n_ids * sizeof(TokenAlts)));
        HIPCHK(launch_records_rows(d_logits_all, plan.n_ids, c.vocab, rec->k, dsc.as<TokenScore>(), dal.as<TokenAlts>(), s));
        if (rec->scores) HIPCHK(hipMemcpyAsync(rec->scores, dsc.p, (size_t)plan.n_ids * sizeof(TokenScore), hipMemcpyDeviceToHost, s));
        if (rec->alts) HIPCHK(hipMemcpyAsync(rec->alts, dal.p, (size_t)plan.n_ids * sizeof(TokenAlts), hipMemcpyDeviceToHost, s));
    }
    const bool eng_used = eng && plan.steps > 0;
    if (eng_used) VOXCHK(engine_err_enqueue(m, m->eng_offline.err_word, s));
    HIPCHK(hipStreamSynchronize(s));
    stage.end();
    *eng_timed_out = eng_used && m->eng_offline.err_word[0] != 0;
    return VOX_OK;
}

// transcribe_streaming on device-resident mel [n_mels][T]  (gguf/model.rs:873-963): encode, plan, attempt, the re-run policy, bookkeeping.
// from_padded_samples: d_mel is the log-mel of samples the library itself padded (vox_transcribe_audio) -- the only case in which the model's prefix state stands for the
// first encoder rows and decoder positions (a caller's own mel may hold anything there).
static int32_t transcribe_dev(vox_model* m, const float* d_mel, int T, const float* t_embed, int32_t* out_ids, int32_t cap, int32_t* n_ids,
                              float* logits_host, bool from_padded_samples = false, const ClipRecords* rec = nullptr) {
    VOXCHK(vox_model_set_t_embed(m, t_embed));
    const bool pfx = from_padded_samples && !logits_host && !rec && prefix_usable(m, T);      // (prefix_build ran before the mel was made: vox_transcribe_audio; records are taken from the kept logits rows: the tap's plan)
    double t0 = now_ms();
    RoctxScope whole("transcribe_streaming");
    int S = 0; RoctxStage stage; stage.begin("encode_audio");
    VOXCHK(encode_dev(m, d_mel, T, &S, pfx ? m->pfx.RC : 0));
    HIPCHK(hipStreamSynchronize(m->ctx->stream));                       // e2e_bench.rs:161-167 forces a sync here too
    stage.end();
    m->timings.encode_ms = now_ms() - t0; t0 = now_ms();
    *n_ids = 0; m->timings.decode_tokens = 0; m->timings.graph_replays = 0;
    const ClipPlan plan = plan_clip(S, pfx, m->pfx.PC, logits_host != nullptr || rec != nullptr);
    if (plan.n_ids == 0) { m->timings.decode_ms = 0; return VOX_OK; }
    ARGCHK(cap >= plan.n_ids, "out_ids capacity %d < %d", cap, plan.n_ids);
    bool timed_out = false;
    VOXCHK(clip_attempt(m, plan, out_ids, logits_host, rec, &timed_out));
    if (timed_out) {
        // A bounded hand-off wait expired inside the engine: its 256 workgroups were not co-resident for 20 ms (another kernel on the GPU, a CU mask, a debugger).  The ids
        // of that attempt are not trustworthy -- the SAME utterance is decoded again on the per-operator launches (the encoder output is still in place), the engine is
        // re-armed for the next utterance, and after three strikes it is switched off for the life of the model.
        const unsigned e = m->eng_offline.err_word[0];
        VOXCHK(engine_strike(m));
        fprintf(stderr, "[voxtral_hip] decode engine: %s; this utterance is decoded again on the per-operator path%s\n",
                engine_timeout_text(e, m->eng_strikes).c_str(), m->eng_strikes >= 3 ? ", the engine is switched off" : "");
        int32_t r; { EngSuspend off(m); r = clip_attempt(m, plan, out_ids, logits_host, rec, &timed_out); }
        graphs_destroy(m);      // (the graph captured during the re-run holds the per-operator launches)
        if (r != VOX_OK) return r;
    }
    m->cache->len = plan.first_pos + plan.steps;
    *n_ids = plan.n_ids; m->timings.decode_tokens = plan.n_ids;
    m->timings.decode_ms = now_ms() - t0;
    return VOX_OK;
}

extern "C" int32_t vox_encode_audio(vox_model* m, const float* mel, int32_t T, float* out, int32_t cap_rows, int32_t* S, int32_t mem_kind) {
    ARGCHK(m && mel && out && S, "null argument"); ARGCHK(T > 0, "empty mel"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    const float* d_mel = mel;
    if (mem_kind == VOX_MEM_HOST) {
        VOXCHK(ensure(&m->d_mel, &m->mel_cap, (size_t)c.n_mels * T));
        HIPCHK(hipMemcpyAsync(m->d_mel, mel, (size_t)c.n_mels * T * 4, hipMemcpyHostToDevice, s)); d_mel = m->d_mel;
    }
    int S4 = 0; VOXCHK(encode_dev(m, d_mel, T, &S4));
    ARGCHK(cap_rows >= S4, "output capacity %d rows < %d", cap_rows, S4);
    if (S4 > 0) HIPCHK(hipMemcpyAsync(out, m->d_audio, (size_t)S4 * c.dec_dim * 4, mem_kind == VOX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    *S = S4; return VOX_OK;
}

extern "C" int32_t vox_transcribe_streaming(vox_model* m, const float* mel, int32_t T, const float* t_embed, int32_t* out_ids, int32_t cap,
                                            int32_t* n_ids, float* logits, int32_t mem_kind) {
    ARGCHK(m && mel && t_embed && out_ids && n_ids, "null argument"); ARGCHK(T > 0, "empty mel"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    const float* d_mel = mel;
    m->timings = vox_timings{};
    if (mem_kind == VOX_MEM_HOST) {
        VOXCHK(ensure(&m->d_mel, &m->mel_cap, (size_t)c.n_mels * T));
        HIPCHK(hipMemcpyAsync(m->d_mel, mel, (size_t)c.n_mels * T * 4, hipMemcpyHostToDevice, s)); d_mel = m->d_mel;
    }
    VOXCHK(transcribe_dev(m, d_mel, T, t_embed, out_ids, cap, n_ids, logits));
    m->timings.total_ms = m->timings.preprocess_ms + m->timings.encode_ms + m->timings.decode_ms;
    return VOX_OK;
}

// the single clip's front end on the context's stream, no synchronisation: samples up (host), peak scale into the context's cell (peak_normalize(0.95), transcribe.rs:207),
// (virtual) pad + log-mel [128][*T_out] into m->d_mel
static int32_t clip_front_end(vox_model* m, const float* samples, size_t n, int32_t mem_kind, int* T_out) {
    vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const float* d_s = samples;
    if (mem_kind == VOX_MEM_HOST) {
        VOXCHK(ensure(&m->d_samples, &m->samples_cap, n));
        HIPCHK(hipMemcpyAsync(m->d_samples, samples, n * 4, hipMemcpyHostToDevice, s)); d_s = m->d_samples;
    }
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    const size_t left = pad_left(&pc), right = pad_right(&pc, n + left), total = left + n + right, T = total / 160;
    MelTables t; VOXCHK(ctx_mel_tables(cx, &t));
    VOXCHK(ensure(&m->d_mel, &m->mel_cap, (size_t)128 * T));
    HIPCHK(launch_absmax(d_s, (long)n, 0.95f, cx->d_scale, s));
    HIPCHK(launch_mel(d_s, (long)n, (long)left, (long)right, cx->d_scale, t, m->d_mel, (int)T, 1, s));
    *T_out = (int)T;
    return VOX_OK;
}
// what the scored entry points check of their record arguments, before a device is touched: k in 0 .. 8, alts exactly when k >= 1, at least one array
static int32_t records_args_check(const void* scores, const void* alts, int32_t k) {
    ARGCHK(k >= 0 && k <= VOX_MAX_ALTERNATIVES, "k %d out of range (0..%d)", k, VOX_MAX_ALTERNATIVES);
    ARGCHK(k > 0 || !alts, "alts given with k == 0: k in 1..%d asks for alternatives", VOX_MAX_ALTERNATIVES);
    ARGCHK(k == 0 || alts, "k %d needs the alts array", k);
    ARGCHK(scores || alts, "scores and alts are both null: the unscored call serves that");
    return VOX_OK;
}
static int32_t transcribe_audio_impl(vox_model* m, const float* samples, size_t n, const float* t_embed, int32_t* out_ids, int32_t cap,
                                     int32_t* n_ids, int32_t mem_kind, const ClipRecords* rec);
extern "C" int32_t vox_transcribe_audio(vox_model* m, const float* samples, size_t n, const float* t_embed, int32_t* out_ids, int32_t cap,
                                        int32_t* n_ids, int32_t mem_kind) {
    return transcribe_audio_impl(m, samples, n, t_embed, out_ids, cap, n_ids, mem_kind, nullptr);
}
extern "C" int32_t vox_transcribe_audio_scored(vox_model* m, const float* samples, size_t n, const float* t_embed, int32_t* out_ids, int32_t cap, int32_t* n_ids,
                                               vox_token_score* scores, vox_token_alts* alts, int32_t k, int32_t mem_kind) {
    ARGCHK(m, "null model"); ARGCHK(samples && t_embed && out_ids, "null argument"); ARGCHK(n_ids, "null n_ids"); ARGCHK(n > 0, "empty audio");
    VOXCHK(records_args_check(scores, alts, k));
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    const ClipRecords rec{scores, alts, k};
    return transcribe_audio_impl(m, samples, n, t_embed, out_ids, cap, n_ids, mem_kind, &rec);
}
static int32_t transcribe_audio_impl(vox_model* m, const float* samples, size_t n, const float* t_embed, int32_t* out_ids, int32_t cap,
                                     int32_t* n_ids, int32_t mem_kind, const ClipRecords* rec) {
    ARGCHK(m && samples && t_embed && out_ids && n_ids, "null argument"); ARGCHK(n > 0, "empty audio"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    ARGCHK(c.n_mels == 128, "the log-mel front-end produces 128 bins; model expects %d", c.n_mels);
    m->timings = vox_timings{};
    VOXCHK(prefix_build(m, t_embed));      // nothing to do once the model holds its prefix state for this t_embed (the first call of a model pays it, outside the stage times)
    const double t0 = now_ms();
    int T = 0; VOXCHK(clip_front_end(m, samples, n, mem_kind, &T));
    HIPCHK(hipStreamSynchronize(s));
    m->timings.preprocess_ms = now_ms() - t0;
    VOXCHK(transcribe_dev(m, m->d_mel, T, t_embed, out_ids, cap, n_ids, nullptr, true, rec));
    m->timings.total_ms = m->timings.preprocess_ms + m->timings.encode_ms + m->timings.decode_ms;
    return VOX_OK;
}

// ---- batched transcription (BASELINE config "Batch=16 x 16 s"; the reference has no batch API: its callers loop) -------------
// Every utterance runs the whole hot path; encode + 38-token prefill are per utterance, the decode loop is batched: one step
// advances all sequences (rows of one skinny MFMA GEMM per linear, so the Q4 weights are streamed once per step for the
// whole batch), per-sequence positions / KV-cache slices / audio rows live on the device, the step is hipGraph-replayed.
static const int32_t VOX_RETRY_ON_LAUNCHES = -1000;      // internal: a batched engine timed out; the driver's caller serves the call again on the launch-based step
// run(allow_engine): one driver call; a call whose engine timed out is served again on the launch-based step
template <class Run> static int32_t retry_on_launches(Run run) { int32_t r = run(true); if (r == VOX_RETRY_ON_LAUNCHES) r = run(false); return r; }
// Both batched drivers run every chain of a decode step back to back on the session stream, eager or captured (until the corpus crash fix they forked the chains onto
// side streams: hipGraphLaunch of a graph with parallel branches reads past the end of its stream list when one shares the launch stream's hardware queue, a host crash).
// declared after a driver's pooled buffers: on every exit path the streams that may still use them are drained before the buffers go back to the pool
struct BatchDrain { vox_ctx* c; ~BatchDrain() { (void)hipStreamSynchronize(c->stream); if (c->fe_stream) (void)hipStreamSynchronize(c->fe_stream); } };
// sequence lengths of a batch, a pure function of the sample count (pad.rs + mel.rs:175-182 + conv.rs:47-48 + adapter.rs:114): T mel frames, S positions, len the
// positions to decode up to (0: shorter than the prefix, emits nothing, model.rs:887-889; S == 38 still writes tokens[38], model.rs:922-926); checks the caller's capacities
static int32_t batch_lengths(const vox_model* m, int n, const float* const* samples, const size_t* n_samples, const int32_t* caps, const int* slot_of,
                             std::vector<int>& T, std::vector<int>& S, std::vector<int>& len, int* Smax) {
    const int PREFIX_LEN = VOX_PREFIX_TOKENS;
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    T.assign(n, 0); S.assign(n, 0); len.assign(n, 0); *Smax = 0;
    for (int i = 0; i < n; i++) {
        ARGCHK(samples[i] && n_samples[i] > 0, "empty audio in batch slot %d", slot_of[i]);
        const size_t left = pad_left(&pc), total = left + n_samples[i] + pad_right(&pc, n_samples[i] + left);
        T[i] = (int)(total / 160); S[i] = conv_len(conv_len(T[i])) / m->cfg.reshape_factor; *Smax = std::max(*Smax, S[i]);
        const int cnt_i = S[i] >= PREFIX_LEN ? std::max(S[i] - PREFIX_LEN, 1) : 0;
        ARGCHK(caps[i] >= cnt_i, "out_ids[%d] capacity %d < %d", slot_of[i], caps[i], cnt_i);
        len[i] = S[i] >= PREFIX_LEN ? std::max(S[i], PREFIX_LEN + 1) : 0;
    }
    ARGCHK(*Smax <= m->dec_rope_len, "sequence too long for the decoder RoPE table");
    return VOX_OK;
}
// front-end of units i0 .. i0 + nu - 1 on stream sf, no host synchronisation: samples up (smp non-null: the samples are host memory, packed into smp), peak-normalise
// (unit_scale null: the unit's own peak into scale[k]), log-mel packed into mel; d_mels[k] = unit i0 + k's log-mel
static int32_t front_end_units(const MelTables& mt, int i0, int nu, const float* const* samples, const size_t* n_samples, const int* T, const float* const* unit_scale,
                               float* smp, float* mel, float* scale, const float** d_mels, hipStream_t sf) {
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    size_t mo = 0, so = 0;
    for (int k = 0; k < nu; k++) {
        const int i = i0 + k; const float* d_s = samples[i];
        if (smp) { float* dst = smp + so; so += n_samples[i]; HIPCHK(hipMemcpyAsync(dst, samples[i], n_samples[i] * 4, hipMemcpyHostToDevice, sf)); d_s = dst; }
        const size_t left = pad_left(&pc), right = pad_right(&pc, n_samples[i] + left);
        float* mel_i = mel + mo; mo += (size_t)128 * T[i]; d_mels[k] = mel_i;
        if (!unit_scale) HIPCHK(launch_absmax(d_s, (long)n_samples[i], 0.95f, scale + k, sf));
        HIPCHK(launch_mel(d_s, (long)n_samples[i], (long)left, (long)right, unit_scale ? unit_scale[i] : scale + k, mt, mel_i, T[i], 1, sf));
    }
    return VOX_OK;
}
// prefix tokens (BOS + STREAMING_PAD), first positions (the prefix's last row) and sequence lengths of n utterances up to the device (gguf/model.rs:887-902)
static int32_t upload_prefix(int n, int tstride, const std::vector<int>& len, int* d_tok, int* d_pos, int* d_len, hipStream_t s) {
    std::vector<int32_t> prefix((size_t)n * tstride, 0); std::vector<int> pos0(n, VOX_PREFIX_TOKENS - 1);
    for (int i = 0; i < n; i++) std::copy(PREFIX_TOKENS.t, PREFIX_TOKENS.t + VOX_PREFIX_TOKENS, prefix.begin() + (size_t)i * tstride);
    HIPCHK(hipMemcpyAsync(d_tok, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(d_pos, pos0.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));      // the host vectors go out of scope
    return VOX_OK;
}
// every utterance's generated ids (tokens[38 ..]; S == 38 still emits its first token, model.rs:922-926) into the caller's arrays; *total = their number
static int32_t copy_out_ids(int n, const std::vector<int>& S, int tstride, const int* d_tok, int32_t* const* out_ids, int32_t* n_ids, int* total, hipStream_t s) {
    const int PREFIX_LEN = VOX_PREFIX_TOKENS;
    std::vector<int32_t> host_tok((size_t)n * tstride);
    HIPCHK(hipMemcpyAsync(host_tok.data(), d_tok, host_tok.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s)); *total = 0;
    for (int i = 0; i < n; i++) {
        const int cnt = S[i] >= PREFIX_LEN ? std::max(S[i] - PREFIX_LEN, 1) : 0;
        if (cnt > 0) std::memcpy(out_ids[i], host_tok.data() + (size_t)i * tstride + PREFIX_LEN, (size_t)cnt * 4);
        n_ids[i] = cnt; *total += cnt;
    }
    return VOX_OK;
}
// Drains s, reads the hand-off error words of the first n_blk engine state blocks.  A hand-off wait that expired inside an engine launch (it needs all 256 CUs to itself) makes
// the call's ids untrustworthy: say so, return VOX_RETRY_ON_LAUNCHES (the caller serves the call again on the launch-based step); three strikes switch the batched engine off.
static int32_t engb_timeout_check(vox_model* m, int n_blk, bool continuous, hipStream_t s) {
    for (int b = 0; b < n_blk; b++) { EngBParams ep{}; engb_state_carve(m->engb_state[b], &ep); HIPCHK(hipMemcpyAsync(m->engb_err_host[b], ep.err, 8, hipMemcpyDeviceToHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < n_blk; b++) if (m->engb_err_host[b][0]) {
        const unsigned e = m->engb_err_host[b][0];
        m->engb_strikes++;
        char grp[32] = ""; if (!continuous) snprintf(grp, sizeof grp, ", group %d", b);
        fprintf(stderr, "[voxtral_hip] batched decode engine%s: hand-off timeout (code %u, workgroup %u%s), strike %d of 3; re-running the %s on the launch-based step%s\n",
                continuous ? " (continuous batch)" : "", e & 0xff, (e >> 8) & 0xff, grp, m->engb_strikes, continuous ? "session" : "batch", m->engb_strikes >= 3 ? ", the engine is switched off" : "");
        for (int gj = 0; gj < 4; gj++) if (m->engb_state[gj]) (void)engb_state_init(m->engb_state[gj], s);
        if (m->engb_strikes >= 3) m->engb_ok = false;      // (otherwise re-armed for the next call)
        return VOX_RETRY_ON_LAUNCHES;      // (the caller runs the call again once this attempt's buffers and graphs are back in the pool: ADVICE r4 -- no recursion from inside the driver)
    }
    return VOX_OK;
}
// One instantiated graph per set of active groups of a batched decode loop.  A step is one chain of kernels on `s`, so the destructor drains `s` alone.
struct StepGraphs {
    hipStream_t s; std::vector<std::pair<uint32_t, hipGraphExec_t>> ex; std::vector<hipGraph_t> gr;
    explicit StepGraphs(hipStream_t st) : s(st) {} StepGraphs(const StepGraphs&) = delete; StepGraphs& operator=(const StepGraphs&) = delete;
    ~StepGraphs() { (void)hipStreamSynchronize(s); for (auto& e : ex) if (e.second) (void)hipGraphExecDestroy(e.second); for (auto g : gr) if (g) (void)hipGraphDestroy(g); }
    hipGraphExec_t find(uint32_t a) const { for (auto& e : ex) if (e.first == a) return e.second; return nullptr; }
    template <class Step> int32_t capture(uint32_t act, Step& step, hipGraphExec_t* out) {      // records step(act) on s as act's graph
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int32_t r = step(act);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        if (graph) gr.push_back(graph);
        if (r != VOX_OK) return r;
        HIPCHK(ce);
        const hipError_t ie = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
        if (ie != hipSuccess) return fail(VOX_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
        ex.emplace_back(act, *out);
        return VOX_OK;
    }
};
// XF planes of one 16-row group over K columns: bf16 hi + lo in MFMA A-operand order
static size_t xf_bytes(int K) { return (size_t)2 * (K / 128) * 256 * 16; }

// ---- one decode attention launch on host buffers (tests): the AttnParams of the batched steps (xf_chain; the lock-step per-operator step; n_seq == 1: the single-row
// step's with the position per sequence), ONE launch through launch_attn_decode (slab) or launch_attn_decode_paged (page_rows > 0).  Which kernel ran is the launchers'
// choice alone (vox_debug_attn_launches).  Every argument is checked before the context is bound -- the positions against the cache, the cache slices against n_slices,
// every table entry of a sequence's window against the pool: nothing a kernel reads lies outside the uploaded buffers.
extern "C" int32_t vox_debug_attn_gqa_max_seq(vox_ctx* c, int32_t* out) {
    ARGCHK(c && out, "null argument"); VOXCHK(ctx_bind(c));
    int most = 0; HIPCHK(attn_decode_gqa_max_seq(&most));
    *out = most; return VOX_OK;
}
// ring: vox_debug_attn_decode_ring -- the slab call's buffers with the cache slices used as rings of max_seq rows (launch_attn_decode_ring)
// tab_len > 0: vox_debug_attn_decode_paged_ring -- the paged call with every table row used as a ring of tab_len entries (AttnParams::page_tab_len), positions to 2^24 - 1
// bf16: vox_debug_attn_decode_paged_bf16 -- the paged call (flat or ring table) on uint16_t pools of the same layout (AttnParams::kv_bf16)
static int32_t attn_decode_debug(vox_ctx* c, const vox_attn_decode_desc* d, const float* q, const void* k, const void* v, void* out, bool ring, int tab_len = 0, bool bf16 = false) {
    ARGCHK(c && d && q && k && v && out, "null argument"); ARGCHK(d->pos, "null argument (pos)");
    ARGCHK(d->head_dim == 128, "head_dim %d: the decoder's decode attention serves head_dim 128 alone", d->head_dim);
    ARGCHK(d->n_seq >= 1 && d->n_seq <= 4096, "n_seq %d out of range (1..4096)", d->n_seq);
    ARGCHK(d->n_heads >= 1 && d->n_kv_heads >= 1 && d->n_heads <= 64 && d->n_heads % d->n_kv_heads == 0, "bad head counts (%d query heads, %d KV heads)", d->n_heads, d->n_kv_heads);
    ARGCHK(d->window >= -1, "window %d (-1: none)", d->window);
    ARGCHK(d->n_slices >= 1 && d->n_slices <= 4096 && (d->kv_row || d->n_slices >= d->n_seq), "n_slices %d: without kv_row every sequence reads its own slice (n_seq %d)", d->n_slices, d->n_seq);
    for (int i = 0; d->kv_row && i < d->n_seq; i++) ARGCHK(d->kv_row[i] >= 0 && d->kv_row[i] < d->n_slices, "kv_row[%d] = %d outside the %d slices", i, d->kv_row[i], d->n_slices);
    const bool paged = d->page_rows != 0;
    const int hd = 128, H = d->n_heads, KV = d->n_kv_heads, QD = H * hd, W = QD + 2 * KV * hd, n = d->n_seq;
    int shift = 0;
    if (ring) {
        ARGCHK(d->max_seq >= 1 && d->max_seq <= 16384, "max_seq %d (the ring capacity) out of range (1..16384)", d->max_seq);
        ARGCHK(!paged && !d->pool_pages && !d->page_tab && !d->page_tab_stride && !d->score_rows, "a ring call takes no paged field");
        ARGCHK(!d->prefer_gqa && !d->spec && !d->out_xf, "the ring form is the per-head kernel writing f32 rows: prefer_gqa, spec and out_xf must be 0");
        ARGCHK(d->window >= 0 && d->window + 1 <= d->max_seq, "window %d: a ring of %d rows serves windows 0..%d", d->window, d->max_seq, d->max_seq - 1);
        for (int i = 0; i < n; i++) ARGCHK(d->pos[i] >= 0 && d->pos[i] < (1 << 24), "pos[%d] = %d outside 0..2^24 - 1", i, d->pos[i]);
    } else if (!paged) {
        ARGCHK(d->max_seq >= 1 && d->max_seq <= 16384, "max_seq %d out of range (1..16384)", d->max_seq);
        ARGCHK(!d->pool_pages && !d->page_tab && !d->page_tab_stride && !d->score_rows, "a slab call takes no paged field");
        for (int i = 0; i < n; i++) ARGCHK(d->pos[i] >= 0 && d->pos[i] < d->max_seq, "pos[%d] = %d outside the cache's %d rows", i, d->pos[i], d->max_seq);
    } else {
        ARGCHK(d->page_rows >= 16 && d->page_rows <= 1024 && !(d->page_rows & (d->page_rows - 1)), "page_rows %d is not a power of two in 16..1024", d->page_rows);
        while ((1 << shift) < d->page_rows) shift++;
        ARGCHK(d->page_tab, "null argument (page_tab)"); ARGCHK(!d->max_seq && !d->spec, "a paged call takes no max_seq and has no speculative form");
        ARGCHK(d->pool_pages >= 1 && d->pool_pages <= (1 << 20), "pool_pages %d out of range", d->pool_pages);
        ARGCHK(d->page_tab_stride >= 1 && d->page_tab_stride <= 1024, "page_tab_stride %d out of range (1..1024)", d->page_tab_stride);
        ARGCHK(d->score_rows >= 1 && d->score_rows <= 16384, "score_rows %d out of range (1..16384)", d->score_rows);
        if (tab_len) {      // the window's keys touch at most window / page_rows + 2 pages; a ring table also holds the two a call may enter ahead of a release
            ARGCHK(d->window >= 0, "a ring table needs a sliding window (window %d)", d->window);
            ARGCHK(tab_len <= d->page_tab_stride, "page_tab_len %d exceeds page_tab_stride %d", tab_len, d->page_tab_stride);
            ARGCHK(tab_len >= d->window / d->page_rows + 2 + 2, "page_tab_len %d: a window of %d in pages of %d rows needs a ring table of at least %d entries (the window's %d pages + 2)", tab_len,
                   d->window, d->page_rows, d->window / d->page_rows + 4, d->window / d->page_rows + 2);
        }
        for (int i = 0; i < n; i++) {
            const int pos = d->pos[i], row = d->kv_row ? d->kv_row[i] : i;
            if (tab_len) ARGCHK(pos >= 0 && pos < (1 << 24), "pos[%d] = %d outside 0..2^24 - 1", i, pos);
            else
            ARGCHK(pos >= 0 && (pos >> shift) < d->page_tab_stride, "pos[%d] = %d outside the table's %d pages of %d rows", i, pos, d->page_tab_stride, d->page_rows);
            const int j_lo = d->window >= 0 ? std::max(0, pos - d->window) : 0;
            ARGCHK(pos - j_lo + 1 <= d->score_rows, "pos[%d] = %d attends %d keys, score_rows is %d", i, pos, pos - j_lo + 1, d->score_rows);
            for (int pg = j_lo >> shift; pg <= (pos >> shift); pg++) {
                const int e = d->page_tab[(size_t)row * d->page_tab_stride + (tab_len ? pg % tab_len : pg)];
                ARGCHK(e >= 0 && e < d->pool_pages, "sequence %d: table entry %d of its window is %d, outside the pool's %d pages", i, pg, e, d->pool_pages);
            }
        }
    }
    VOXCHK(ctx_bind(c));
    if (!paged && d->prefer_gqa && attn_decode_takes_gqa(hd, H, KV)) {      // (the one check that needs the device: the kernel's attributes)
        int most = 0; HIPCHK(attn_decode_gqa_max_seq(&most));
        ARGCHK(d->max_seq <= most, "max_seq %d: the slab GQA form serves at most %d rows per KV head", d->max_seq, most);
    }
    hipStream_t s = c->stream;
    const size_t slice_f = paged ? (size_t)KV * d->page_rows * hd : (size_t)KV * d->max_seq * hd, kv_f = slice_f * (paged ? d->pool_pages : d->n_slices);
    const int n_grp = (n + 15) / 16; const size_t xf_b = xf_bytes(QD);
    DevBuf dq, dk, dv, dout, dxf, dint;
    const size_t tab_n = paged ? (size_t)d->n_slices * d->page_tab_stride : 0;
    const size_t kv_b = kv_f * (bf16 ? 2 : 4);
    HIPCHK(dq.alloc((size_t)n * W * 4)); HIPCHK(dk.alloc(kv_b)); HIPCHK(dv.alloc(kv_b)); HIPCHK(dout.alloc((size_t)n * QD * 4)); HIPCHK(dxf.alloc(xf_b * n_grp));
    HIPCHK(dint.alloc((2 * (size_t)n + tab_n) * 4));
    int* d_pos = dint.as<int>(); int* d_row = d_pos + n; int* d_tab = d_row + n;
    HIPCHK(hipMemsetAsync(dq.p, 0, (size_t)n * W * 4, s));
    HIPCHK(hipMemcpy2DAsync(dq.p, (size_t)W * 4, q, (size_t)QD * 4, (size_t)QD * 4, n, hipMemcpyHostToDevice, s));      // q rows at the q|k|v row stride, as the steps hold them
    HIPCHK(hipMemcpyAsync(dk.p, k, kv_b, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dv.p, v, kv_b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pos, d->pos, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (d->kv_row) HIPCHK(hipMemcpyAsync(d_row, d->kv_row, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (paged) HIPCHK(hipMemcpyAsync(d_tab, d->page_tab, tab_n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dout.p, 0xff, (size_t)n * QD * 4, s));      // a row the launch does not write stays NaN
    HIPCHK(hipMemsetAsync(dxf.p, 0, xf_b * n_grp, s));                 // (the planes of a step start zeroed: XfPlanes)
    AttnParams ap{}; ap.q = dq.as<float>(); ap.k = dk.as<float>(); ap.v = dv.as<float>(); ap.kv_row_stride = hd; ap.kv_head_stride = d->max_seq * hd; ap.n_heads = H; ap.n_kv_heads = KV;
    ap.offset = 0; ap.window = d->window; ap.pos_ptr = d_pos; ap.M = 1; ap.pos_per_seq = 1; ap.q_seq_stride = W; ap.out_seq_stride = QD; ap.kv_seq_stride = (long)slice_f;
    ap.kv_row = d->kv_row ? d_row : nullptr; ap.prefer_gqa = d->prefer_gqa != 0; ap.no_xcd_remap = d->no_xcd_remap != 0; ap.spec_rows = d->spec ? d->max_seq : 0;
    ap.out = dout.as<float>(); if (d->out_xf) { ap.out_xf = dxf.as<uint16_t>(); ap.out_xf_gstride = (long)(xf_b / 2); }
    if (paged) {
        ap.kv_head_stride = (hd << shift); ap.page_tab = d_tab; ap.page_tab_stride = d->page_tab_stride; ap.page_shift = shift; ap.page_floats = (long)slice_f; ap.score_rows = d->score_rows;
        ap.page_tab_len = tab_len; ap.kv_bf16 = bf16 ? 1 : 0;
        HIPCHK(launch_attn_decode_paged(ap, hd, s, n));
    } else if (ring) HIPCHK(launch_attn_decode_ring(ap, hd, d->max_seq, s, n));
    else HIPCHK(launch_attn_decode(ap, hd, d->max_seq, s, n));
    if (d->out_xf) HIPCHK(hipMemcpyAsync(out, dxf.p, xf_b * n_grp, hipMemcpyDeviceToHost, s));
    else HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * QD * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
extern "C" int32_t vox_debug_attn_decode(vox_ctx* c, const vox_attn_decode_desc* d, const float* q, const float* k, const float* v, void* out) {
    return attn_decode_debug(c, d, q, k, v, out, false);
}
extern "C" int32_t vox_debug_attn_decode_ring(vox_ctx* c, const vox_attn_decode_desc* d, const float* q, const float* k, const float* v, void* out) {
    return attn_decode_debug(c, d, q, k, v, out, true);
}
extern "C" int32_t vox_debug_attn_decode_paged_ring(vox_ctx* c, const vox_attn_decode_desc* d, int32_t page_tab_len, const float* q, const float* k, const float* v, void* out) {
    ARGCHK(d, "null argument"); ARGCHK(d->page_rows != 0, "a ring table belongs to a paged call (page_rows 0)");
    ARGCHK(page_tab_len >= 1 && page_tab_len <= 1024, "page_tab_len %d out of range (1..1024)", page_tab_len);
    return attn_decode_debug(c, d, q, k, v, out, false, page_tab_len);
}
extern "C" int32_t vox_debug_attn_decode_paged_bf16(vox_ctx* c, const vox_attn_decode_desc* d, int32_t page_tab_len, const float* q, const uint16_t* k, const uint16_t* v, void* out) {
    ARGCHK(d, "null argument"); ARGCHK(d->page_rows != 0, "a bf16 pool belongs to a paged call (page_rows 0)");
    ARGCHK(page_tab_len >= 0 && page_tab_len <= 1024, "page_tab_len %d out of range (0: a flat table; 1..1024: a ring table)", page_tab_len);
    ARGCHK(d->page_rows >= 16 && d->page_rows <= 1024 && !(d->page_rows & (d->page_rows - 1)), "page_rows %d is not a power of two in 16..1024", d->page_rows);
    if (page_tab_len) {      // (attn_decode_debug's ring-table conditions, stated here as well: they hold whatever else the call passes)
        ARGCHK(d->window >= 0, "a ring table needs a sliding window (window %d)", d->window);
        ARGCHK(page_tab_len >= d->window / d->page_rows + 4, "page_tab_len %d: a window of %d in pages of %d rows needs a ring table of at least %d entries", page_tab_len, d->window, d->page_rows,
               d->window / d->page_rows + 4);
    }
    return attn_decode_debug(c, d, q, k, v, out, false, page_tab_len, true);
}
// ---- one launch of the live sessions' encoder ring attention on host buffers (tests): the StreamAttnParams of stream_encode_round -- StreamMember descriptors on the
// device with state[STRM_ENC_POS], kring and vring alone filled in, the order array, the caller's q|k|v rows, the RoPE rows as a flat table (the model's streaming
// table), one RoPE ring (a solo endless session's: stream_rope_refill) or a ring per member (an endless group's: group_rope_refill) -- and ONE launch_stream_attn.  The
// RoPE rows come from rope_rows_fill with vox_debug_rope_rows' table length, so a test holds the identical f32 rows; in the ring modes only the rows the served members'
// positions need are written, every other ring row is NaN.  Every argument is checked before the context is bound: what launch_stream_attn refuses never reaches it, and
// nothing the kernel reads or writes lies outside the uploaded buffers (order against n_members, the positions against the table or 2^24, the ring offset against layers).
// burst: vox_debug_stream_attn_burst -- rows up to 64, and the ONE launch is launch_stream_attn_burst
// rows_per_slot (vox_debug_stream_attn_group_burst; null: every slot has d->rows rows): slot z has rows_per_slot[z] rows, a multiple of 4 in 4..64, d->rows is the
// largest of them; qkv and out hold the slots' rows back to back, and the ONE launch is launch_stream_attn_group_burst with rpt = 4
static int32_t stream_attn_debug(vox_ctx* c, const vox_stream_attn_desc* d, const float* qkv, float* kring, float* vring, float* out, bool burst, const int32_t* rows_per_slot = nullptr) {
    ARGCHK(c && d && qkv && kring && vring && out, "null argument"); ARGCHK(d->order && d->enc_pos, "null argument (order, enc_pos)");
    ARGCHK(d->head_dim == 64 || d->head_dim == 128, "head_dim %d: the ring attention serves head_dim 64 and 128", d->head_dim);
    const int max_rows = burst ? 64 : 8;
    ARGCHK(d->rows >= 1 && d->rows <= max_rows, "rows %d out of range (1..%d)", d->rows, max_rows);
    ARGCHK(d->n_slots >= 1 && d->n_slots <= 16, "n_slots %d out of range (1..16)", d->n_slots);
    ARGCHK(d->n_members >= d->n_slots && d->n_members <= 64, "n_members %d out of range (n_slots = %d .. 64)", d->n_members, d->n_slots);
    ARGCHK(d->n_heads >= 1 && d->n_heads <= 32, "n_heads %d out of range (1..32)", d->n_heads);
    ARGCHK(d->window >= 0 && d->window + 1 <= 1024, "window %d: the kernel holds 1024 scores, windows 0..1023", d->window);
    ARGCHK(d->cap > d->window + d->rows && d->cap <= 16384, "cap %d: a ring holds window + rows < cap <= 16384 rows (window %d, rows %d)", d->cap, d->window, d->rows);
    ARGCHK(d->layers >= 1 && d->layers <= 8 && d->layer >= 0 && d->layer < d->layers, "layer %d of %d layers (1..8)", d->layer, d->layers);
    ARGCHK(std::isfinite(d->theta) && d->theta > 1.0f, "theta %g must be finite and above 1", (double)d->theta);
    const int R = d->rope_rows, M = d->rows, n = d->n_slots, NM = d->n_members;
    StreamBurstDesc bd{}; int rows_all = n * M, slot_rows[16];      // the rows of qkv / out, and of every slot
    for (int z = 0; z < n; z++) slot_rows[z] = M;
    if (rows_per_slot) {
        int most = 0; rows_all = 0;
        for (int z = 0; z < n; z++) {
            const int mz = rows_per_slot[z];
            ARGCHK(mz >= 4 && mz <= 64 && mz % 4 == 0, "rows_per_slot[%d] = %d: a slot of a burst round has 4 b rows, b in 1..16", z, mz);
            slot_rows[z] = mz; bd.tick0[z] = rows_all / 4; bd.b[z] = mz / 4; rows_all += mz; most = std::max(most, mz);
        }
        ARGCHK(most == M, "rows %d is not the largest of rows_per_slot (%d)", M, most);
    }
    // (a ring of one row would have the mask 0, which the kernel reads as "a flat table")
    ARGCHK(R == 0 || (R >= 2 && R >= M && R <= 4096 && !(R & (R - 1))), "rope_rows %d: a RoPE ring has a power of two of rows, at least `rows` (%d) and 2, at most 4096", R, M);
    ARGCHK(R || !d->rope_per_member, "rope_per_member without a RoPE ring (rope_rows 0)");
    const int64_t pos_end = R ? ((int64_t)1 << 24) : (int64_t)ROPE_ENC_STREAM_TABLE_LEN;
    for (int i = 0; i < NM; i++)
        ARGCHK(d->enc_pos[i] >= 0 && (int64_t)d->enc_pos[i] + M <= pos_end, "enc_pos[%d] = %d: the %d rows of a tick end at position %lld here", i, d->enc_pos[i], M, (long long)pos_end);
    bool served[64] = {};
    for (int z = 0; z < n; z++) {
        ARGCHK(d->order[z] >= 0 && d->order[z] < NM, "order[%d] = %d outside the %d members", z, d->order[z], NM);
        ARGCHK(!served[d->order[z]], "order[%d] = %d: a member is served by one slot", z, d->order[z]);
        served[d->order[z]] = true;
    }
    const bool per_member = R && d->rope_per_member;
    const int hd = d->head_dim, half = hd / 2, H = d->n_heads, QD = H * hd;
    const int64_t table_len = rope_debug_table_len(hd);
    // the RoPE rows, on the host
    std::vector<float> rope; size_t sin_at = 0;
    if (!R) {
        int64_t T = 0; for (int z = 0; z < n; z++) T = std::max<int64_t>(T, (int64_t)d->enc_pos[d->order[z]] + M);
        rope.resize((size_t)2 * T * half); sin_at = (size_t)T * half;
        rope_rows_fill(hd, d->theta, 0, T, table_len, nullptr, rope.data(), rope.data() + sin_at);
    } else {
        rope.assign((size_t)(per_member ? NM : 1) * R * hd, std::nanf("")); sin_at = (size_t)half;
        std::vector<int64_t> holds((size_t)(per_member ? NM : 1) * R, -1);
        for (int z = 0; z < n; z++) for (int r = 0; r < slot_rows[z]; r++) {
            const int64_t p = (int64_t)d->enc_pos[d->order[z]] + r; const size_t row = (per_member ? (size_t)d->order[z] * R : 0) + (size_t)(p & (R - 1));
            ARGCHK(holds[row] < 0 || holds[row] == p, "one RoPE ring of %d rows cannot hold positions %lld and %lld (slot %d): rope_per_member gives every member its own", R, (long long)holds[row], (long long)p, z);
            holds[row] = p;
            rope_rows_fill(hd, d->theta, p, 1, table_len, nullptr, rope.data() + row * hd, rope.data() + row * hd + half);
        }
    }
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream;
    const size_t layer_f = (size_t)H * d->cap * hd, mem_f = (size_t)d->layers * layer_f, ring_f = (size_t)NM * mem_f, qkv_f = (size_t)rows_all * 3 * QD, out_f = (size_t)rows_all * QD;
    DevBuf dqkv, dk, dv, dout, drope, dint, dmem, ddesc;
    HIPCHK(dqkv.alloc(qkv_f * 4)); HIPCHK(dk.alloc(ring_f * 4)); HIPCHK(dv.alloc(ring_f * 4)); HIPCHK(dout.alloc(out_f * 4)); HIPCHK(drope.alloc(rope.size() * 4));
    HIPCHK(dint.alloc(((size_t)NM * STRM_WORDS + n) * 4)); HIPCHK(dmem.alloc((size_t)NM * sizeof(StreamMember)));
    int* d_state = dint.as<int>(); int* d_order = d_state + (size_t)NM * STRM_WORDS;
    std::vector<int> state((size_t)NM * STRM_WORDS, 0); std::vector<StreamMember> mem((size_t)NM, StreamMember{});
    for (int i = 0; i < NM; i++) {
        state[(size_t)i * STRM_WORDS + STRM_ENC_POS] = d->enc_pos[i];
        mem[i].state = d_state + (size_t)i * STRM_WORDS; mem[i].kring = dk.as<float>() + (size_t)i * mem_f; mem[i].vring = dv.as<float>() + (size_t)i * mem_f;
    }
    HIPCHK(hipMemcpyAsync(dqkv.p, qkv, qkv_f * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dk.p, kring, ring_f * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dv.p, vring, ring_f * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(drope.p, rope.data(), rope.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_state, state.data(), state.size() * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(d_order, d->order, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dmem.p, mem.data(), mem.size() * sizeof(StreamMember), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dout.p, 0xff, out_f * 4, s));      // a row the launch does not write stays NaN
    StreamAttnParams ap{}; ap.qkv = dqkv.as<float>(); ap.qkv_stride = 3 * QD; ap.mem = dmem.as<StreamMember>(); ap.order = d_order; ap.n = n; ap.ring_off = (size_t)d->layer * layer_f; ap.cap = d->cap;
    ap.cos_t = drope.as<float>(); ap.sin_t = drope.as<float>() + sin_at; ap.out = dout.as<float>(); ap.out_stride = QD; ap.M = M; ap.n_heads = H; ap.window = d->window;
    ap.rope_mask = R ? R - 1 : 0; ap.rope_stride = per_member ? R : 0;
    if (rows_per_slot) {
        HIPCHK(ddesc.alloc(sizeof(StreamBurstDesc))); HIPCHK(hipMemcpyAsync(ddesc.p, &bd, sizeof(StreamBurstDesc), hipMemcpyHostToDevice, s));
        HIPCHK(launch_stream_attn_group_burst(ap, ddesc.as<StreamBurstDesc>(), bd, 4, hd, s));
    } else HIPCHK(burst ? launch_stream_attn_burst(ap, hd, s) : launch_stream_attn(ap, hd, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, out_f * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(kring, dk.p, ring_f * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(vring, dv.p, ring_f * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
extern "C" int32_t vox_debug_stream_attn(vox_ctx* c, const vox_stream_attn_desc* d, const float* qkv, float* kring, float* vring, float* out) {
    return stream_attn_debug(c, d, qkv, kring, vring, out, false);
}
// the burst form of the same attention (a burst stream's encoder layers, b >= 2): vox_debug_stream_attn's arguments and checks with rows 1..64, ONE launch_stream_attn_burst
extern "C" int32_t vox_debug_stream_attn_burst(vox_ctx* c, const vox_stream_attn_desc* d, const float* qkv, float* kring, float* vring, float* out) {
    return stream_attn_debug(c, d, qkv, kring, vring, out, true);
}
// the RAGGED burst form (a burst group's round): the same arguments and checks, plus rows_per_slot[n_slots] -- ONE launch_stream_attn_group_burst
extern "C" int32_t vox_debug_stream_attn_group_burst(vox_ctx* c, const vox_stream_attn_desc* d, const int32_t* rows_per_slot, const float* qkv, float* kring, float* vring, float* out) {
    ARGCHK(rows_per_slot, "null argument");
    return stream_attn_debug(c, d, qkv, kring, vring, out, true, rows_per_slot);
}
extern "C" int32_t vox_debug_stream_attn_burst_launches(uint64_t* out) {
    ARGCHK(out, "null argument");
    *out = (uint64_t)stream_attn_burst_launches();
    return VOX_OK;
}
// the seeding of a session's rings from the prefix state on host buffers (tests): ONE launch_stream_ring_init into the caller's rings
extern "C" int32_t vox_debug_stream_ring_init(vox_ctx* c, int32_t layers, int32_t rows, int32_t n_heads, int32_t head_dim, int32_t cap, const float* kv, float* kring, float* vring) {
    ARGCHK(c && kv && kring && vring, "null argument");
    ARGCHK(head_dim == 64 || head_dim == 128, "head_dim %d: the encoder rings hold head_dim 64 or 128", head_dim);
    ARGCHK(layers >= 1 && layers <= 64 && n_heads >= 1 && n_heads <= 64, "%d layers of %d heads out of range (1..64 each)", layers, n_heads);
    ARGCHK(cap >= 1 && cap <= 16384, "cap %d out of range (1..16384)", cap);
    ARGCHK(rows >= 1 && rows <= cap, "rows %d: a ring of %d rows is seeded with 1..%d rows", rows, cap, cap);
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream;
    const size_t kv_f = (size_t)layers * rows * 2 * n_heads * head_dim, ring_f = (size_t)layers * n_heads * cap * head_dim;
    DevBuf dkv, dk, dv;
    HIPCHK(dkv.alloc(kv_f * 4)); HIPCHK(dk.alloc(ring_f * 4)); HIPCHK(dv.alloc(ring_f * 4));
    HIPCHK(hipMemcpyAsync(dkv.p, kv, kv_f * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dk.p, kring, ring_f * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dv.p, vring, ring_f * 4, hipMemcpyHostToDevice, s));
    HIPCHK(launch_stream_ring_init(dkv.as<float>(), layers, rows, n_heads, head_dim, cap, dk.as<float>(), dv.as<float>(), s));
    HIPCHK(hipMemcpyAsync(kring, dk.p, ring_f * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(vring, dv.p, ring_f * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
// the sessions' level kernel on hand-made sessions (tests): ONE launch_stream_level -- the plain form, a solo burst's or a burst round's ragged one -- on uploaded
// rings and state words; every list comes back, the records the launch did not write as (NaN, NaN)
extern "C" int32_t vox_debug_stream_level(vox_ctx* c, int32_t n_members, const float* rings, int32_t ring_n, const float* gains, const int32_t* pos, const int32_t* frame,
                                          const int32_t* order, int32_t n_slots, int32_t ticks, const int32_t* burst_b, int32_t list_len, vox_tick_level* out) {
    ARGCHK(c && rings && gains && pos && frame && order && out, "null argument");
    ARGCHK(n_members >= 1 && n_members <= 16 && n_slots >= 1 && n_slots <= n_members, "%d slots of %d members (1..16, slots <= members)", n_slots, n_members);
    ARGCHK(ring_n >= 4096 && ring_n <= (1 << 20) && !(ring_n & (ring_n - 1)), "ring_n %d: a power of two in 4096 .. 2^20", ring_n);
    ARGCHK(ticks >= 1 && ticks <= VOX_STREAM_BURST_MAX, "ticks %d out of range (1..%d)", ticks, VOX_STREAM_BURST_MAX);
    ARGCHK(list_len >= 1 && list_len <= 65536, "list_len %d out of range (1..65536)", list_len);
    unsigned seen = 0;
    for (int z = 0; z < n_slots; z++) {
        ARGCHK(order[z] >= 0 && order[z] < n_members && !(seen >> order[z] & 1u), "order[%d] = %d: members 0..%d, each once", z, order[z], n_members - 1);
        seen |= 1u << order[z];
        if (burst_b) ARGCHK(burst_b[z] >= 1 && burst_b[z] <= ticks && (z == 0 || burst_b[z] <= burst_b[z - 1]), "burst_b[%d] = %d: 1..%d, descending", z, burst_b[z], ticks);
    }
    for (int i = 0; i < n_members; i++) {
        ARGCHK(pos[i] >= VOX_PREFIX_TOKENS - 1 && pos[i] <= (1 << 24) && frame[i] >= 0 && frame[i] <= (1 << 28), "member %d: position %d, frame %d", i, pos[i], frame[i]);
        ARGCHK(std::isfinite(gains[i]), "member %d: gain is not finite", i);
    }
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream;
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc); const long left = (long)pad_left(&pc);
    const size_t NM = (size_t)n_members, ring_b = NM * ring_n * 4, list_b = NM * list_len * sizeof(TickLevel);
    DevBuf drings, dstate, dlists, dmem, dorder, ddesc;
    HIPCHK(drings.alloc(ring_b)); HIPCHK(dstate.alloc(NM * STRM_WORDS * 4)); HIPCHK(dlists.alloc(list_b)); HIPCHK(dmem.alloc(NM * sizeof(StreamMember))); HIPCHK(dorder.alloc(16 * 4));
    std::vector<int> state(NM * STRM_WORDS, 0); std::vector<StreamMember> mem(NM, StreamMember{}); int h_order[16] = {0};
    for (size_t i = 0; i < NM; i++) {
        state[i * STRM_WORDS + STRM_POS] = pos[i]; state[i * STRM_WORDS + STRM_FRAME] = frame[i];
        mem[i].samples = drings.as<float>() + i * ring_n; mem[i].gain = gains[i]; mem[i].state = dstate.as<int>() + i * STRM_WORDS;
        mem[i].levels = dlists.as<TickLevel>() + i * list_len; mem[i].levels_cap = list_len;
    }
    for (int z = 0; z < n_slots; z++) h_order[z] = order[z];
    StreamBurstDesc bd; std::memset(&bd, 0, sizeof bd);
    if (burst_b) { int t0 = 0; for (int z = 0; z < n_slots; z++) { bd.tick0[z] = t0; bd.b[z] = burst_b[z]; t0 += burst_b[z]; } HIPCHK(ddesc.alloc(sizeof bd)); HIPCHK(hipMemcpyAsync(ddesc.p, &bd, sizeof bd, hipMemcpyHostToDevice, s)); }
    HIPCHK(hipMemcpyAsync(drings.p, rings, ring_b, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dstate.p, state.data(), NM * STRM_WORDS * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dmem.p, mem.data(), NM * sizeof(StreamMember), hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dorder.p, h_order, sizeof h_order, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dlists.p, 0xFF, list_b, s));      // every record (NaN, NaN)
    HIPCHK(launch_stream_level(dmem.as<StreamMember>(), dorder.as<int>(), n_slots, ring_n - 1, left, VOX_PREFIX_TOKENS - 1, ticks, burst_b ? ddesc.as<StreamBurstDesc>() : nullptr, burst_b ? &bd : nullptr, s));
    HIPCHK(hipMemcpyAsync(out, dlists.p, list_b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
// What a batched XF decode step works on.  f32 rows (h, qkv, logits; att unread), XF planes and partial sums of squares one block per 16-row group, `*_gs` elements apart.
// k / v: layer 0's cache slab (layer l at + l layer_stride), row r's slice at + r seq_stride, or, with kv_row, the slice kv_row[r] names; pos: the rows' positions.
// ssq_e: the batched engine's sums of squares (one block of 256 + 16 rows per group); planes: the wide step's K-split scratch, planes_bytes per chain.
struct XfBufs {
    float *h, *qkv, *att, *logits, *ssq; uint16_t *xf1, *xf2, *xf3; long xf1_gs, xf2_gs, xf3_gs, ssq_gs;
    float *k, *v; size_t layer_stride, seq_stride; int max_seq; const int *pos, *kv_row; bool no_xcd_remap;
    float* ssq_e; void* planes; size_t planes_bytes;
    // a paged cache (a paged stream group; null / 0 everywhere else, and the code of a contiguous cache runs): k / v are the page pool [layer][page][kv head][page_rows][hd],
    // page_tab [member][page_tab_stride] its table, kv_row the rows' MEMBERS (attention finds its table row), kv_page / kv_in the rows' physical page and row inside it
    // (the q|k|v epilogue appends there); score_rows: the attention's LDS score rows per query head
    const int *page_tab, *kv_page, *kv_in; int page_tab_stride, page_shift, score_rows; long page_floats;
    // an endless paged group: the table rows are rings of page_tab_len entries, and the q|k|v epilogue reads its RoPE rows from the group's member-strided decoder
    // RoPE ring (rope_ring [members][rope_mask + 1][cos | sin]; the row's member: kv_row).  0 / null everywhere else
    int page_tab_len; const float* rope_ring; int rope_mask;
    // a bf16 pool (a bf16 paged group): k / v point at uint16_t pools, layer_stride and page_floats count 16-bit elements.  0 everywhere else
    int kv_bf16;
    // a stream group with a delay per member: ada_rows [member][dec_layers][dec_dim] every member's Ada scales (ada_stride floats per member), ada_order the rows' members --
    // the wo GEMM's epilogue multiplies row r by member ada_order[r]'s scales (EPI_RESID_XF_ROWS).  null everywhere else: the model's one set, per column
    const float* ada_rows; const int* ada_order; long ada_stride;
};
// the XF planes and ssq blocks of a step over n_grp groups (0: none, the group strides alone): from the pool, zeroed on s, bound to b
struct XfPlanes {
    DevBuf xf1, xf2, xf3, ssq;
    int32_t alloc(const vox_model* m, int n_grp, hipStream_t s, XfBufs* b) {
        const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx;
        const size_t b1 = xf_bytes(c.dec_dim), b2 = xf_bytes(c.dec_heads * c.dec_head_dim), b3 = xf_bytes(c.dec_ffn), bs = (size_t)q4_skinny_resid_xf_parts(c.dec_dim) * 16 * 4;
        b->xf1_gs = (long)(b1 / 2); b->xf2_gs = (long)(b2 / 2); b->xf3_gs = (long)(b3 / 2); b->ssq_gs = (long)(bs / 4);
        if (!n_grp) return VOX_OK;
        HIPCHK(xf1.alloc_pooled(cx, b1 * n_grp)); HIPCHK(xf2.alloc_pooled(cx, b2 * n_grp)); HIPCHK(xf3.alloc_pooled(cx, b3 * n_grp)); HIPCHK(ssq.alloc_pooled(cx, bs * n_grp));
        HIPCHK(hipMemsetAsync(xf1.p, 0, b1 * n_grp, s)); HIPCHK(hipMemsetAsync(xf2.p, 0, b2 * n_grp, s)); HIPCHK(hipMemsetAsync(xf3.p, 0, b3 * n_grp, s));
        HIPCHK(hipMemsetAsync(ssq.p, 0, bs * n_grp, s));
        b->xf1 = xf1.as<uint16_t>(); b->xf2 = xf2.as<uint16_t>(); b->xf3 = xf3.as<uint16_t>(); b->ssq = ssq.as<float>();
        return VOX_OK;
    }
};
// One chain of an XF decode step on stream sg: 4 launches per layer and the lm_head (RMSNorm folded into producers and consumers, RoPE + KV-cache write in the q|k|v
// GEMM's epilogue).  mtw == 0: ONE 16-row group, rows 16 g0i .. 16 g0i + ng - 1 of the buffers, through launch_q4_gemm.  mtw = 2..4 (the WIDE chain, round 6): the slot
// groups g0i .. g0i + mtw - 1 as ONE GEMM per operator (launch_q4_wide: one weight fetch and one nibble -> bf16 conversion per K step for all groups, the groups' XF
// planes staged through LDS once per workgroup, K split over workgroups + a finishing launch with the step's epilogue), their attention in one launch, the lm_head as one
// GEMM; `chain`: which slice of the planes scratch.  The fields only launch_q4_wide reads are set on that path alone.
static int32_t xf_chain(const vox_model* m, const XfBufs& b, int g0i, int ng, int mtw, int chain, bool prefer_gqa, int spec_rows, hipStream_t sg) {
    const vox_model_cfg& c = m->cfg;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, W = QD + 2 * KV * hd, F = c.dec_ffn, V = c.vocab;
    const int parts_D = q4_skinny_resid_xf_parts(D), max_seq = b.max_seq, M = mtw ? 16 * mtw : ng;
    ARGCHK(!(b.page_tab && mtw), "internal: a paged cache runs the one-group chain (the wide step has no paged form)");
    ARGCHK(!b.kv_bf16 || b.page_tab, "internal: a bf16 K/V pool is a paged cache's");
    ARGCHK(!b.ada_rows || (!mtw && b.ada_order), "internal: Ada scales per row run the one-group chain, with the rows' members");
    const int r0 = g0i * 16;      // the chain's first group: its planes, sums, rows, positions and cache slices (a wide chain's further groups follow at the group strides)
    uint16_t* xf1 = b.xf1 + (size_t)g0i * b.xf1_gs; uint16_t* xf2 = b.xf2 + (size_t)g0i * b.xf2_gs; uint16_t* xf3 = b.xf3 + (size_t)g0i * b.xf3_gs; float* ssq = b.ssq + (size_t)g0i * b.ssq_gs;
    float* hg = b.h + (size_t)r0 * D; float* qg = b.qkv + (size_t)r0 * W; const int* pg = b.pos + r0; const int* rg = b.kv_row ? b.kv_row + r0 : nullptr;
    const size_t row0 = b.kv_row ? 0 : (size_t)r0 * b.seq_stride;
    auto gemm = [&](GemmParams g, const Q4W& w, const uint16_t* xin, int K, int epi) -> hipError_t {      // g: the operator's epilogue fields
        xf_step_bind(g, w, xin, M, epi, c.norm_eps, mtw, reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(b.planes) + (size_t)chain * b.planes_bytes), b.planes_bytes,
                     (long)(xf_bytes(K) / 2), epi == EPI_SWIGLU_XF ? b.xf3_gs : b.xf1_gs, b.ssq_gs, b.ssq_gs);
        return xf_step_launch(g, epi, sg);
    };
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayer& L = m->dec[l];
        float* kl = b.k + (size_t)l * b.layer_stride + row0; float* vl = b.v + (size_t)l * b.layer_stride + row0;
        if (b.kv_bf16) {      // (a paged pool: row0 is 0) the layer's pages, in 16-bit elements
            kl = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(b.k) + (size_t)l * b.layer_stride); vl = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(b.v) + (size_t)l * b.layer_stride);
        }
        { GemmParams g{}; xf_fill_rope_kv(g, qg, W, ssq, l == 0 ? 1 : parts_D, pg, m->dec_cos, m->dec_sin, hd, QD, KV, kl, vl, (long)b.seq_stride, max_seq, rg);
          if (b.page_tab) xf_fill_rope_kv_paged(g, b.page_floats, 1 << b.page_shift, b.kv_page + r0, b.kv_in + r0, b.kv_bf16);
          if (b.page_tab && b.rope_ring) xf_fill_rope_ring(g, b.rope_ring, rg, b.rope_mask);
          HIPCHK(gemm(g, L.wqkv.w, xf1, D, EPI_ROPE_KV)); }
        AttnParams ap{}; ap.q = qg; ap.k = kl; ap.v = vl; ap.kv_row_stride = hd; ap.kv_head_stride = max_seq * hd; ap.n_heads = H; ap.n_kv_heads = KV;
        ap.offset = 0; ap.window = c.dec_window; ap.pos_ptr = pg; ap.M = 1; ap.pos_per_seq = 1; ap.q_seq_stride = W; ap.out_seq_stride = QD; ap.kv_seq_stride = (long)b.seq_stride;
        ap.kv_row = rg; ap.out_xf = xf2; ap.prefer_gqa = prefer_gqa; ap.no_xcd_remap = b.no_xcd_remap; ap.spec_rows = spec_rows;
        ap.out = b.att; if (mtw) { ap.out = b.att + (size_t)g0i * 16 * QD; ap.out_xf_gstride = b.xf2_gs; }
        if (b.page_tab) {
            ap.kv_head_stride = (hd << b.page_shift); ap.page_tab = b.page_tab; ap.page_tab_stride = b.page_tab_stride; ap.page_shift = b.page_shift; ap.page_floats = b.page_floats;
            ap.score_rows = b.score_rows; ap.page_tab_len = b.page_tab_len; ap.kv_bf16 = b.kv_bf16;
            HIPCHK(launch_attn_decode_paged(ap, hd, sg, M));
        } else
        HIPCHK(launch_attn_decode(ap, hd, max_seq, sg, M));
        { GemmParams g{}; xf_fill_resid_xf(g, hg, hg, D, xf1, L.ffn_norm, L.ada_mul, ssq);
          if (b.ada_rows) { g.xf_w2 = b.ada_rows + (size_t)l * D; g.xf_w2_row = b.ada_order; g.xf_w2_stride = b.ada_stride; }      // every row its member's scales
          HIPCHK(gemm(g, L.wo.w, xf2, QD, EPI_RESID_XF)); }
        { GemmParams g{}; xf_fill_swiglu_xf(g, xf3, F, ssq, parts_D); HIPCHK(gemm(g, L.w13.w, xf1, D, EPI_SWIGLU_XF)); }
        { GemmParams g{}; xf_fill_resid_xf(g, hg, hg, D, xf1, l + 1 < c.dec_layers ? m->dec[l + 1].attn_norm : m->dec_norm, nullptr, ssq); HIPCHK(gemm(g, L.w2.w, xf3, F, EPI_RESID_XF)); }
    }
    { GemmParams g{}; xf_fill_store(g, b.logits + (size_t)g0i * 16 * V, V, ssq, parts_D); HIPCHK(gemm(g, m->tok.w, xf1, D, EPI_STORE)); }
    return VOX_OK;
}
// The batched decode-layer engine's parameters for group gi (n_rows of its 16): layer table `tab`, edge-buffer block `blk` (a block belongs to a launch, not to a
// group: tags carry the block's launch serial), `two`: one half of a two-group launch.  Cache slices per slot when b.kv_row is set.
static EngBParams engb_params(const vox_model* m, const XfBufs& b, int gi, int n_rows, int tab, int blk, bool two) {
    const vox_model_cfg& c = m->cfg; const int r0 = gi * 16;
    EngBParams ep{}; ep.stream = m->eng_stream; ep.stream_wo = m->eng_wob; ep.layers = m->engb_tab[tab]; ep.n_layers = c.dec_layers; ep.kv_seq_stride = (long)b.seq_stride;
    ep.h_in = b.h + (size_t)r0 * c.dec_dim; ep.h_stride = c.dec_dim; ep.n_rows = n_rows; ep.final_norm = m->dec_norm; ep.pos = b.pos + r0; ep.kv_row = b.kv_row ? b.kv_row + r0 : nullptr;
    ep.rope_cos = m->dec_cos; ep.rope_sin = m->dec_sin; ep.max_seq = b.max_seq; ep.window = c.dec_window; ep.eps = c.norm_eps;
    engb_state_carve(m->engb_state[blk], &ep);
    ep.xf_out = b.xf1 + (size_t)gi * b.xf1_gs; ep.ssq_out = b.ssq_e + (size_t)gi * (256 + 16) * 16; ep.tl = nullptr; ep.tl_layer = -1; ep.flags = two ? m->engb_flags2 : m->engb_flags;
    return ep;
}
// after a batched engine launch: group gi's 256 partial sums of squares (b.ssq_e) -> 16, then its lm_head over ng rows
static int32_t engb_group_tail(const vox_model* m, const XfBufs& b, int gi, int ng, hipStream_t s) {
    float* ssq_p = b.ssq_e + (size_t)gi * (256 + 16) * 16; float* ssq_f = ssq_p + 256 * 16;
    HIPCHK(launch_engb_ssq_fold(ssq_p, ssq_f, s));
    GemmParams g{}; g.w = m->tok.w; g.xf = (const uint4*)(b.xf1 + (size_t)gi * b.xf1_gs); g.M = ng; g.out = b.logits + (size_t)gi * 16 * m->cfg.vocab; g.out_stride = m->cfg.vocab;
    g.ssq_part = ssq_f; g.n_part = 16; g.norm_eps = m->cfg.norm_eps; HIPCHK(launch_q4_gemm(g, EPI_STORE, s));
    return VOX_OK;
}
static bool batch_xf_ok(const vox_model* m) {
    const vox_model_cfg& c = m->cfg; const int D = c.dec_dim, QD = c.dec_heads * c.dec_head_dim, F = c.dec_ffn;
    return m->tok.w.fmt == WFMT_Q4_0 && m->dec[0].wqkv.w.fmt == WFMT_Q4_0 && m->tok.w.qt && m->dec[0].wqkv.w.qt && D % 128 == 0 && QD % 128 == 0 && F % 128 == 0 && !knob_str("VOX_BATCH_NO_XF");
}
// the logits tap of one driver call (vox_debug_batch_tap_*): clip_unit[i] = the tap index of the driver's utterance i (slot_of[i] = its caller index), or -1.  Off:
// no buffer, no launch.  rows(...) enqueues the copy of the rows the next argmax launch reads (launch_batch_tap), inside a capture as well as eagerly.
struct BatchTapCall {
    vox_model* m; DevBuf clip_unit; int n = 0;
    bool on() const { return clip_unit.p != nullptr; }
    int32_t init(vox_model* mm, int nn, const int* slot_of, hipStream_t s) {
        m = mm; n = nn;
        if (!m->tap.on) return VOX_OK;
        std::vector<int> cu(n, -1); bool any = false;
        for (int i = 0; i < n; i++) for (size_t j = 0; j < m->tap.units.size(); j++) if (m->tap.units[j] == slot_of[i]) { cu[i] = (int)j; any = true; }
        if (!any) return VOX_OK;
        HIPCHK(clip_unit.alloc_pooled(m->ctx, (size_t)n * 4));
        HIPCHK(hipMemcpyAsync(clip_unit.p, cu.data(), (size_t)n * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipStreamSynchronize(s));      // (cu goes out of scope)
        return VOX_OK;
    }
    int32_t rows(const float* logits, int n_rows, const int* slot_clip, int clip0, const int* pos, const int* seq_len, hipStream_t s) const {
        if (!on()) return VOX_OK;
        BatchTapParams p{}; p.logits = logits; p.vocab = m->cfg.vocab; p.slot_clip = slot_clip; p.clip0 = clip0; p.pos = pos; p.seq_len = seq_len;
        p.clip_unit = (const int*)clip_unit.p; p.n_clips = n; p.out = m->tap.out; p.rows = m->tap.rows; p.n_units = (int)m->tap.units.size(); p.max_rows = m->tap.max_rows;
        p.first_pos = VOX_PREFIX_TOKENS;
        HIPCHK(launch_batch_tap(p, n_rows, s));
        return VOX_OK;
    }
};
// What a scored batch call asked for (vox_transcribe_batch_scored): per-unit host arrays in the order of the call's units (either may be null; unit i's hold caps[i]
// entries) and k.  The drivers permute and slice these as they do out_ids.
struct RecordsOut { vox_token_score* const* scores; vox_token_alts* const* alts; int k; };
// The records of one driver call (launch_batch_records): utterance i's record j lives at rec_off[i] + j of one device array per kind, rec_off = the prefix sum of the
// planned id counts (batch_lengths: a pure function of the sample counts).  Off (no RecordsOut): no buffer, no launch.  rows(...) enqueues the records of the rows the
// next argmax launch reads, inside a capture as well as eagerly, at BatchTapCall::rows' three sites; download(...) goes in front of the call's last synchronisation
// (copy_out_ids'), scatter() behind it: the first n_ids records of every unit into the caller's arrays, nothing past them.
struct BatchRecordsCall {
    vox_model* m = nullptr; const RecordsOut* out = nullptr; int n = 0;
    DevBuf off, sc, al; std::vector<int> h_off; std::vector<TokenScore> h_sc; std::vector<TokenAlts> h_al;
    bool on() const { return out != nullptr; }
    int total() const { return h_off.empty() ? 0 : h_off.back(); }
    int32_t init(vox_model* mm, int nn, const std::vector<int>& S, const RecordsOut* o, hipStream_t s) {
        m = mm; n = nn; out = o;
        if (!on()) return VOX_OK;
        h_off.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; i++) h_off[(size_t)i + 1] = h_off[i] + (S[i] >= VOX_PREFIX_TOKENS ? std::max(S[i] - VOX_PREFIX_TOKENS, 1) : 0);      // copy_out_ids' counts
        HIPCHK(off.alloc_pooled(m->ctx, h_off.size() * 4));
        HIPCHK(hipMemcpyAsync(off.p, h_off.data(), h_off.size() * 4, hipMemcpyHostToDevice, s));
        if (out->scores) HIPCHK(sc.alloc_pooled(m->ctx, (size_t)total() * sizeof(TokenScore)));
        if (out->alts) HIPCHK(al.alloc_pooled(m->ctx, (size_t)total() * sizeof(TokenAlts)));
        HIPCHK(hipStreamSynchronize(s));      // (no pageable copy may sit behind the stages that follow)
        return VOX_OK;
    }
    int32_t rows(const float* logits, int n_rows, const int* slot_clip, int clip0, const int* pos, const int* seq_len, hipStream_t s) const {
        if (!on() || total() == 0) return VOX_OK;
        BatchRecordsParams p{}; p.logits = logits; p.vocab = m->cfg.vocab; p.slot_clip = slot_clip; p.clip0 = clip0; p.pos = pos; p.seq_len = seq_len;
        p.rec_off = (const int*)off.p; p.n_clips = n; p.n_records = total(); p.first_pos = VOX_PREFIX_TOKENS;
        p.scores = (TokenScore*)sc.p; p.alts = (TokenAlts*)al.p; p.k = out->k;
        HIPCHK(launch_batch_records(p, n_rows, s));
        return VOX_OK;
    }
    int32_t download(hipStream_t s) {
        if (!on() || total() == 0) return VOX_OK;
        if (out->scores) { h_sc.resize((size_t)total()); HIPCHK(hipMemcpyAsync(h_sc.data(), sc.p, h_sc.size() * sizeof(TokenScore), hipMemcpyDeviceToHost, s)); }
        if (out->alts) { h_al.resize((size_t)total()); HIPCHK(hipMemcpyAsync(h_al.data(), al.p, h_al.size() * sizeof(TokenAlts), hipMemcpyDeviceToHost, s)); }
        return VOX_OK;
    }
    void scatter() const {
        if (!on() || total() == 0) return;
        for (int i = 0; i < n; i++) {
            const size_t o = (size_t)h_off[i], cnt = (size_t)(h_off[(size_t)i + 1] - h_off[i]);
            if (cnt && out->scores) std::memcpy(out->scores[i], h_sc.data() + o, cnt * sizeof(TokenScore));
            if (cnt && out->alts) std::memcpy(out->alts[i], h_al.data() + o, cnt * sizeof(TokenAlts));
        }
    }
};
// Stacked 38-token prefill of nc utterances (gguf/model.rs:887-919) on s: x0[i][r] = audio[aoff[i]][r] + embed(tok[i][r]) into px, the decoder over all nc x 38 rows
// against the cache slices k / v (utterance i's at + i seq_stride), then the logits of every utterance's last prefix row (RMSNorm -> xn, lm_head -> logits): what its
// first generated token is taken from.  Utterances shorter than the prefix emit nothing (model.rs:887-889) -- they ride along as idle rows.
static int32_t prefill_first_logits(vox_model* m, int nc, const int* tok, int tstride, const float* audio, const long* aoff, float* px, float* k, float* v, int max_seq,
                                    size_t layer_stride, size_t seq_stride, float* xn, float* logits, hipStream_t s) {
    const vox_model_cfg& c = m->cfg; const int D = c.dec_dim, PREFIX_LEN = VOX_PREFIX_TOKENS;
    for (int i = 0; i < nc; i++)
        HIPCHK(launch_embed(m->tok.w, tok + (size_t)i * tstride, PREFIX_LEN, audio + aoff[i], D, nullptr, 0, 0, px + (size_t)i * PREFIX_LEN * D, s));
    vox_cache view; view.m = m; view.ctx = m->ctx; view.k = k; view.v = v; view.max_seq = max_seq; view.len = 0; view.layer_stride = layer_stride;
    VOXCHK(decoder_prefill_dev(m, px, nc * PREFIX_LEN, &view, 0, nc, (long)seq_stride));
    HIPCHK(launch_rms_norm(px + (size_t)(PREFIX_LEN - 1) * D, PREFIX_LEN * D, nc, D, m->dec_norm, nullptr, c.norm_eps, xn, D, s));
    { GemmParams g{}; g.w = m->tok.w; g.x = xn; g.x_stride = D; g.M = nc; g.out = logits; g.out_stride = c.vocab; HIPCHK(launch_q4_gemm(g, EPI_STORE, s)); }
    return VOX_OK;
}
// the lock-step step of a model the XF step does not cover: n f32 rows through every layer and the lm_head (xn, act: normalised rows, FFN rows)
static int32_t f32_batch_layers(const vox_model* m, const XfBufs& b, int n, float* xn, float* act, hipStream_t s) {
    const vox_model_cfg& c = m->cfg;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, W = QD + 2 * KV * hd, F = c.dec_ffn, max_seq = b.max_seq;
    float* h = b.h;
    for (int l = 0; l < c.dec_layers; l++) {
        const DecLayer& L = m->dec[l]; float* kl = b.k + (size_t)l * b.layer_stride; float* vl = b.v + (size_t)l * b.layer_stride;
        HIPCHK(launch_rms_norm(h, D, n, D, L.attn_norm, nullptr, c.norm_eps, xn, D, s));
        { GemmParams g{}; g.w = L.wqkv.w; g.x = xn; g.x_stride = D; g.M = n; g.out = b.qkv; g.out_stride = W; HIPCHK(launch_q4_gemm(g, EPI_STORE, s)); }
        HIPCHK(launch_rope_kv_batch(b.qkv, n, W, QD, KV, hd, b.pos, m->dec_cos, m->dec_sin, kl, vl, (long)b.seq_stride, max_seq * hd, s));
        AttnParams ap{}; ap.q = b.qkv; ap.k = kl; ap.v = vl; ap.kv_row_stride = hd; ap.kv_head_stride = max_seq * hd; ap.out = b.att; ap.n_heads = H; ap.n_kv_heads = KV;
        ap.offset = 0; ap.window = c.dec_window; ap.pos_ptr = b.pos; ap.M = 1; ap.pos_per_seq = 1; ap.q_seq_stride = W; ap.out_seq_stride = QD;
        ap.kv_seq_stride = (long)b.seq_stride; ap.spec_rows = max_seq;
        HIPCHK(launch_attn_decode(ap, hd, max_seq, s, n));
        { GemmParams g{}; g.w = L.wo.w; g.x = b.att; g.x_stride = QD; g.M = n; g.out = h; g.out_stride = D; g.resid = h; g.resid_stride = D; HIPCHK(launch_q4_gemm(g, EPI_RESID, s)); }
        HIPCHK(launch_rms_norm(h, D, n, D, L.ffn_norm, L.ada_mul, c.norm_eps, xn, D, s));
        { GemmParams g{}; g.w = L.w13.w; g.x = xn; g.x_stride = D; g.M = n; g.out = act; g.out_stride = F; HIPCHK(launch_q4_gemm(g, EPI_SWIGLU, s)); }
        { GemmParams g{}; g.w = L.w2.w; g.x = act; g.x_stride = F; g.M = n; g.out = h; g.out_stride = D; g.resid = h; g.resid_stride = D; HIPCHK(launch_q4_gemm(g, EPI_RESID, s)); }
    }
    HIPCHK(launch_rms_norm(h, D, n, D, m->dec_norm, nullptr, c.norm_eps, xn, D, s));
    { GemmParams g{}; g.w = m->tok.w; g.x = xn; g.x_stride = D; g.M = n; g.out = b.logits; g.out_stride = c.vocab; HIPCHK(launch_q4_gemm(g, EPI_STORE, s)); }
    return VOX_OK;
}
static int32_t transcribe_batch_impl(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const float* t_embed,
                                     int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind, const int* slot_of, bool allow_engine = true,
                                     const float* const* unit_scale = nullptr, const RecordsOut* rec_out = nullptr) {
    // unit_scale[i]: device float the front-end multiplies unit i by (vox_transcribe_batch_ex: the peak scale of the unit's FILE); null = every unit normalises itself
    // slot_of[i]: the caller's slot of row i (error messages)
    VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    ARGCHK(c.n_mels == 128, "the log-mel front-end produces 128 bins; model expects %d", c.n_mels);
    const int PREFIX_LEN = VOX_PREFIX_TOKENS;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, KD = KV * hd, W = QD + 2 * KD, F = c.dec_ffn, V = c.vocab;
    VOXCHK(vox_model_set_t_embed(m, t_embed));
    m->timings = vox_timings{};
    MelTables mt; VOXCHK(ctx_mel_tables(cx, &mt));
    std::vector<int> S, T, len; int Smax = 0;
    VOXCHK(batch_lengths(m, n, samples, n_samples, caps, slot_of, T, S, len, &Smax));
    const int max_seq = std::max((Smax + 63) / 64 * 64, 64), tstride = std::max(Smax, PREFIX_LEN) + 2;
    const int audio_rows = std::max(enc_row_budget(m, T.data(), n) / c.reshape_factor, PREFIX_LEN + 1);   // per-utterance row budget of the stacked audio embeddings
    const size_t seq_stride = (size_t)KV * max_seq * hd, layer_stride = (size_t)n * seq_stride;
    size_t mel_floats = 0; for (int i = 0; i < n; i++) mel_floats += (size_t)128 * T[i];
    DevBuf b_audio, b_k, b_v, b_tok, b_pos, b_len, b_h, b_xn, b_qkv, b_att, b_act, b_logits, b_px, b_mel, b_scale, b_smp; XfPlanes xfp;
    BatchTapCall tap; VOXCHK(tap.init(m, n, slot_of, s));
    BatchRecordsCall rec; VOXCHK(rec.init(m, n, S, rec_out, s));
    BatchDrain drain{cx};
    HIPCHK(b_audio.alloc_pooled(cx, (size_t)n * audio_rows * D * 4)); HIPCHK(b_k.alloc_pooled(cx, layer_stride * c.dec_layers * 4)); HIPCHK(b_v.alloc_pooled(cx, layer_stride * c.dec_layers * 4));
    HIPCHK(b_tok.alloc_pooled(cx, (size_t)n * tstride * 4)); HIPCHK(b_pos.alloc_pooled(cx, (size_t)n * 4)); HIPCHK(b_len.alloc_pooled(cx, (size_t)n * 4));
    HIPCHK(b_h.alloc_pooled(cx, (size_t)n * D * 4)); HIPCHK(b_xn.alloc_pooled(cx, (size_t)n * D * 4)); HIPCHK(b_qkv.alloc_pooled(cx, (size_t)n * W * 4)); HIPCHK(b_att.alloc_pooled(cx, (size_t)n * QD * 4));
    HIPCHK(b_act.alloc_pooled(cx, (size_t)n * F * 4)); HIPCHK(b_logits.alloc_pooled(cx, (size_t)n * V * 4)); HIPCHK(b_px.alloc_pooled(cx, (size_t)n * PREFIX_LEN * D * 4));
    HIPCHK(b_mel.alloc_pooled(cx, std::max<size_t>(mel_floats, 1) * 4)); HIPCHK(b_scale.alloc_pooled(cx, (size_t)n * 4));
    HIPCHK(hipMemsetAsync(b_tok.p, 0, (size_t)n * tstride * 4, s)); HIPCHK(hipMemsetAsync(b_h.p, 0, (size_t)n * D * 4, s));
    HIPCHK(hipMemsetAsync(b_audio.p, 0, (size_t)n * audio_rows * D * 4, s));
    float* d_audio = b_audio.as<float>(); int* d_tok = b_tok.as<int>(); int* d_pos = b_pos.as<int>(); int* d_len = b_len.as<int>(); float* logits = b_logits.as<float>();
    const double t0 = now_ms();
    // (1) front-end per utterance, no host synchronisation in between: peak-normalise -> (virtual) pad -> log-mel
    std::vector<const float*> d_mels(n);
    if (mem_kind == VOX_MEM_HOST) { size_t smp_total = 0; for (int i = 0; i < n; i++) smp_total += n_samples[i]; HIPCHK(b_smp.alloc_pooled(cx, smp_total * 4)); }
    VOXCHK(front_end_units(mt, 0, n, samples, n_samples, T.data(), unit_scale, mem_kind == VOX_MEM_HOST ? b_smp.as<float>() : nullptr, b_mel.as<float>(), b_scale.as<float>(), d_mels.data(), s));
    HIPCHK(hipStreamSynchronize(s)); const double t_pre = now_ms();
    // (2) stacked encoder + adapter: every GEMM once over all utterances' frames
    std::vector<int> S4(n);
    VOXCHK(encode_batch_dev(m, n, d_mels.data(), T.data(), d_audio, audio_rows, S4.data()));
    for (int i = 0; i < n; i++) ARGCHK(S4[i] == S[i], "internal: sequence length mismatch (%d vs %d)", S4[i], S[i]);
    HIPCHK(hipStreamSynchronize(s)); const double t1 = now_ms();
    const double pre_ms = t_pre - t0, enc_ms = t1 - t_pre;
    // (3) stacked 38-token prefill; its lm_head rows -> first generated token + first step input (same tail as a decode step)
    VOXCHK(upload_prefix(n, tstride, len, d_tok, d_pos, d_len, s));
    std::vector<long> aoff(n); for (int i = 0; i < n; i++) aoff[i] = (long)i * audio_rows * D;
    VOXCHK(prefill_first_logits(m, n, d_tok, tstride, d_audio, aoff.data(), b_px.as<float>(), b_k.as<float>(), b_v.as<float>(), max_seq, layer_stride, seq_stride, b_xn.as<float>(), logits, s));
    // (4) batched decode steps
    int steps = 0; for (int i = 0; i < n; i++) steps = std::max(steps, S[i] - PREFIX_LEN - 1);
    // The step's GEMM inputs live as XF fragment planes (bf16 hi+lo in MFMA A-operand order, written once by the producing kernel), so
    // the skinny kernels spend no VALU on conversion and RMSNorm output never exists as f32.  Sequences are processed in groups of
    // 16 rows (one MFMA m-tile); the groups of a layer run back to back so the second group finds the layer's weights in L2 / MALL.
    const bool use_xf = batch_xf_ok(m);
    const int n_grp = (n + 15) / 16;
    XfBufs xb{}; xb.h = b_h.as<float>(); xb.qkv = b_qkv.as<float>(); xb.att = b_att.as<float>(); xb.logits = logits;
    VOXCHK(xfp.alloc(m, use_xf ? n_grp : 0, s, &xb));
    xb.k = b_k.as<float>(); xb.v = b_v.as<float>(); xb.layer_stride = layer_stride; xb.seq_stride = seq_stride; xb.max_seq = max_seq; xb.pos = d_pos; xb.kv_row = nullptr;
    xb.no_xcd_remap = knob_str("VOX_ATTN_NO_XCD") != nullptr;
    // Batched decode-layer ENGINE (vox_engine_b16.hip): the 26 layers of a 16-row group as ONE persistent launch on the single-stream engine's packet stream; the group's
    // 5 x 26 launches remain as the fallback (other geometries, dense checkpoints, VOX_BATCH_ENGINE=0, a hand-off timeout).  The launch owns all 256 CUs, so the groups of
    // a step run back to back -- measured on the 647-clip corpus in 64-clip batches (four groups): 6 770 tok/s against 8 540 for the launch chains, then forked on side
    // streams (profiles/r04_b16_fleurs_engine_vs_launches.txt), so batches wider than one group keep the launches (VOX_BATCH_ENGINE_WIDE=1: engine for every width).
    const bool use_eng = allow_engine && !m->ctx->shared && use_xf && steps > 0 && (n_grp == 1 || knob_str("VOX_BATCH_ENGINE_WIDE")) && engb_prepare(m, n_grp);
    DevBuf b_ssq_e;
    std::vector<EngLayerTab> eng_tabs((size_t)(use_eng ? n_grp : 0) * c.dec_layers);      // (alive until the copies below have run: the call's last synchronisation)
    if (use_eng) {
        HIPCHK(b_ssq_e.alloc_pooled(cx, (size_t)(256 + 16) * 16 * 4 * n_grp)); xb.ssq_e = b_ssq_e.as<float>();
        for (int gi = 0; gi < n_grp; gi++) {
            EngLayerTab* tab = eng_tabs.data() + (size_t)gi * c.dec_layers;
            dec_layer_tab(m, xb.k, xb.v, layer_stride, (size_t)gi * 16 * seq_stride, tab);
            HIPCHK(hipMemcpyAsync(m->engb_tab[gi], tab, sizeof(EngLayerTab) * c.dec_layers, hipMemcpyHostToDevice, s));
        }
    }
    // argmax of every row's logits -> its next token, position + 1, next step input (the XF step, not the engine, which reads the f32 rows: also its folded first RMSNorm)
    const bool gqa = n_grp > 1 || knob_str("VOX_ATTN_GQA");
    auto next_input = [&](bool xf_in, bool first = false) -> int32_t {
        VOXCHK(tap.rows(logits, n, nullptr, 0, d_pos, d_len, s));
        VOXCHK(rec.rows(logits, n, nullptr, 0, d_pos, d_len, s));
        if (!xf_in && !first) HIPCHK(launch_argmax_embed_batch(logits, n, V, d_tok, tstride, d_pos, d_len, m->tok.w, d_audio, (long)audio_rows * D, D, xb.h, s));
        else HIPCHK(launch_argmax_embed_batch(logits, n, V, d_tok, tstride, d_pos, d_len, m->tok.w, d_audio, (long)audio_rows * D, D, xb.h, s,
                                              xf_in ? xb.xf1 : nullptr, xf_in ? m->dec[0].attn_norm : nullptr, xf_in ? xb.ssq : nullptr, xb.xf1_gs, (int)xb.ssq_gs));
        return VOX_OK;
    };
    VOXCHK(next_input(use_xf, true));      // first generated token of every utterance + the first step's input
    // `active`: bit gi = group gi still has a sequence that needs this step.  A group whose sequences have all reached their last position is RETIRED: its layer
    // chain is not launched any more (its rows idle in place in the argmax / embedding kernel, whose token write is guarded by the sequence length) -- a ragged
    // batch pays for each group only as long as that group's longest member runs, not for the batch's longest member in every group.
    // The groups of a step run in LOCK-STEP (one after another on `s`, one argmax / next-input launch for all rows): letting every group replay its own chain of
    // steps on its own stream -- no join, groups drifting freely -- was measured 12 % SLOWER on the 647-clip corpus (8 520 -> 7 630 tok/s,
    // profiles/r03_batch_independent_groups.txt): groups in lock-step find each other's weights in L2 / MALL, drifting groups stream them from HBM once each.
    auto step = [&](uint32_t active) -> int32_t {
        if (!use_xf) { VOXCHK(f32_batch_layers(m, xb, n, b_xn.as<float>(), b_act.as<float>(), s)); return next_input(false); }
        for (int gi = 0; gi < n_grp; gi++) {
            if (!((active >> gi) & 1u)) continue;
            const int ng = std::min(16, n - gi * 16);
            if (!use_eng) { VOXCHK(xf_chain(m, xb, gi, ng, 0, 0, gqa, max_seq, s)); continue; }
            HIPCHK(launch_decode_engine_b16(engb_params(m, xb, gi, ng, gi, gi, false), s));      // the group's 26 layers as one launch, then its lm_head
            VOXCHK(engb_group_tail(m, xb, gi, ng, s));
        }
        return next_input(!use_eng);
    };
    // steps of group gi = those of its longest member; with the rows sorted by length (vox_transcribe_batch does that) the groups retire last to first
    std::vector<int> steps_g(n_grp, 0);
    for (int i = 0; i < n; i++) steps_g[i / 16] = std::max(steps_g[i / 16], S[i] - PREFIX_LEN - 1);
    const bool retire = use_xf && !knob_str("VOX_BATCH_NO_RETIRE");
    auto active_at = [&](int t) { uint32_t a = 0; for (int gi = 0; gi < n_grp; gi++) if (!retire || t < steps_g[gi]) a |= 1u << gi; return a; };
    StepGraphs graphs(s);      // one graph per set of active groups (<= n_grp of them when the rows are sorted), captured when the set first occurs
    int replays = 0;
    const bool no_graph = knob_str("VOX_BATCH_NO_GRAPH") != nullptr;      // measurement knob (profilers)
    for (int t = 0; t < steps; t++) {
        const uint32_t act = active_at(t);
        if (use_eng) m->engb_launches += (unsigned)__builtin_popcount(act);      // (one engine launch per active group)
        if (t == 0 || no_graph) { VOXCHK(step(act)); continue; }         // eager first step
        hipGraphExec_t ge = graphs.find(act);
        if (!ge) { HIPCHK(hipStreamSynchronize(s)); VOXCHK(graphs.capture(act, step, &ge)); }
        if (hipGraphLaunch(ge, s) != hipSuccess) return fail(VOX_ERR_HIP, "hipGraphLaunch failed");
        replays++;
    }
    VOXCHK(engb_timeout_check(m, use_eng ? n_grp : 0, false, s));
    int total = 0;
    VOXCHK(rec.download(s));
    VOXCHK(copy_out_ids(n, S, tstride, d_tok, out_ids, n_ids, &total, s));
    rec.scatter();
    m->timings.preprocess_ms = pre_ms; m->timings.encode_ms = enc_ms; m->timings.decode_ms = now_ms() - t1; m->timings.total_ms = now_ms() - t0;
    m->timings.decode_tokens = total; m->timings.graph_replays = replays;
    if (knob_str("VOX_BATCH_VERBOSE"))
        fprintf(stderr, "[voxtral_hip] lock-step batch: %d rows, %d groups, %d steps, step form %s\n", n, n_grp, steps, use_eng ? "engine" : use_xf ? "xf-chains" : "f32");
    return VOX_OK;
}

// ---- continuous batching (round 5): wide batches -- a rank's whole share of a corpus (BASELINE configs[4]: 81 of the 647 FLEURS utterances at 8 GPUs) in ONE call.
// The launch-based batch above decodes n rows in ceil(n / 16) lock-step groups and a group is as long as its longest member: a ragged 41-clip batch drains through
// one and two half-empty groups at the full per-step cost (the round-4 one-GPU bound on configs[4]: 5.5 x at 8 GPUs).  Here the decode step runs over SLOTS:
//   (A) every utterance is encoded and prefilled up front, in stacked chunks of <= 64 (the weights stream once per chunk): audio rows, a cache slice and the first decode
//       input h0 per utterance stay on the device (212 992 B of K / V per position: 54 MB per utterance at 256 positions -- nothing next to 288 GB);
//   (B) the host plans the whole decode statically -- token counts are a pure function of the sample count, there is no EOS (gguf/model.rs:936-960): utterances are
//       packed longest-processing-time-first onto 16 G slots (G = 1..4 groups, chosen by the measured per-step cost of G lock-step groups), every slot gets its queue;
//   (C) one decode step = the same four launches per layer and group as above, reading positions and CACHE SLICES per slot (GemmParams::kv_row, AttnParams::kv_row),
//       + argmax_embed_slots_kernel, which hands a slot whose utterance just got its last token the next one of its queue in the same launch.  A group retires when its
//       queues are empty.  Rows are independent of their slot, so the ids per utterance are those of every other path (tests/test_gpu_fullsize.py).
// Step cost of G lock-step groups in ms, measured on the FLEURS-like corpus (profiles/r05_continuous_sweep.txt: decode time net of graph captures / steps; 3 interpolated):
// Five to eight groups (80 .. 128 slots, end of round 6): TWO wide chains per step, ceil(n / 2) and floor(n / 2) groups each -- measured (chains then forked) with tools/wide_probe.py
// (profiles/r06_wide_split.txt); only on a context that owns its GPU.
static const double kStepMs[9] = {0.0, 1.84, 2.08, 2.75, 3.15, 3.55, 3.80, 4.35, 4.70};      // (four groups: the wide step, round 6 -- 3.40 on four forked chains)
// ... with the batched decode-layer engine serving the steps of <= 2 active groups (one group: decode_engine_b16_kernel<1>, 1.06 ms + tail; two: the two-group launch,
// 1.60 ms + tail; three and four groups stay on the launch chains -- a two-group launch + a one- or two-group launch back to back: 2.9 / 3.4 ms against 2.75 / 3.40)
static const double kStepMsEng[9] = {0.0, 1.17, 1.77, 2.75, 3.15, 3.55, 3.80, 4.35, 4.70};      // (four groups: the wide step, round 6)
// the wide step's geometry: every decoder layer the shape of layer 0, tile-ordered Q4 copies, no biases, plans for 2 .. 4 groups per chain
static bool wide_geom_ok(const vox_model* m) {
    const vox_model_cfg& c = m->cfg;
    if (c.dec_head_dim != 128 || c.dec_layers < 1) return false;
    const DecLayer& L0 = m->dec[0];
    for (int mtw = 2; mtw <= 4; mtw++) {
        const struct { const Q4W* w; int epi; } ops[5] = {{&L0.wqkv.w, EPI_ROPE_KV}, {&L0.wo.w, EPI_RESID_XF}, {&L0.w13.w, EPI_SWIGLU_XF}, {&L0.w2.w, EPI_RESID_XF}, {&m->tok.w, EPI_STORE}};
        for (auto& o : ops) { WidePlan pl; if (!q4_wide_plan(*o.w, mtw, o.epi, &pl)) return false; }
    }
    for (int l = 0; l < c.dec_layers; l++) { const DecLayer& L = m->dec[l];
        if (L.wqkv.w.N != L0.wqkv.w.N || L.wqkv.w.K != L0.wqkv.w.K || L.w13.w.N != L0.w13.w.N || L.w2.w.K != L0.w2.w.K || !L.wqkv.w.qt || !L.wo.w.qt || !L.w13.w.qt || !L.w2.w.qt || L.wqkv.bias || L.wo.bias || L.w13.bias || L.w2.bias) return false; }
    return true;
}
// planes scratch of one wide chain of up to mt_max groups: the K-split partial sums of the largest layer GEMM (the lm_head splits no K)
static size_t wide_planes_bytes(const vox_model* m, int mt_max) {
    const DecLayer& L0 = m->dec[0]; size_t bytes = 0;
    const struct { const Q4W* w; int epi; } ops[4] = {{&L0.wqkv.w, EPI_ROPE_KV}, {&L0.wo.w, EPI_RESID_XF}, {&L0.w13.w, EPI_SWIGLU_XF}, {&L0.w2.w, EPI_RESID_XF}};
    for (int mtw = 2; mtw <= mt_max; mtw++) for (auto& o : ops) { WidePlan pl; if (q4_wide_plan(*o.w, mtw, o.epi, &pl)) bytes = std::max(bytes, q4_wide_planes_bytes(*o.w, mtw, pl)); }
    return bytes;
}
// Every knob the continuous driver consults, read once per session (cont_policy), and what follows from them once the plan's group count G is known (cont_policy_groups).
struct ContPolicy {
    int chunk = 64;      // utterances per encoder / prefill stack (VOX_BATCH_CHUNK, measurement knob: 128 measured equal to 64, profiles/r05_continuous_sweep.txt)
    int force_G = 0, max_groups = 4;      // VOX_BATCH_SLOT_GROUPS; more than four groups = two wide chains per step (VOX_BATCH_MAX_GROUPS caps it)
    bool shared = false, use_eng = false, calib = true, no_fe_overlap = false, no_graph = false, verbose = false, no_xcd = false, no_wide = false, no_wide_split = false;
    int wide_min = 4, wide_chains = 2;      // VOX_BATCH_WIDE_MIN = 2 / 3: measurement knob and tests; VOX_BATCH_WIDE_CHAINS: measurement knob, more than two chains per step
    int G = 1; bool wide_ok = false, wide_split = false;
};
static ContPolicy cont_policy(vox_model* m, bool allow_engine, bool have_jobs) {
    ContPolicy p; p.shared = m->ctx->shared;
    if (const char* e = knob_str("VOX_BATCH_CHUNK")) p.chunk = std::max(1, std::min(128, atoi(e)));
    if (const char* e = knob_str("VOX_BATCH_SLOT_GROUPS")) p.force_G = std::max(0, std::min(kMaxGroups, atoi(e)));
    p.no_wide = knob_str("VOX_BATCH_NO_WIDE") != nullptr; p.no_wide_split = knob_str("VOX_BATCH_NO_WIDE_SPLIT") != nullptr;
    // more than four groups = two wide chains per step: needs the wide step's geometry and a GPU of its own (on a shared one the other session fills the gaps)
    if (!p.shared && !p.no_wide && !p.no_wide_split && wide_geom_ok(m)) {
        p.max_groups = kMaxGroups; if (const char* e = knob_str("VOX_BATCH_MAX_GROUPS")) p.max_groups = std::max(1, std::min(kMaxGroups, atoi(e)));
    }
    if (p.force_G > p.max_groups) p.force_G = p.max_groups;
    // the steps of one or two active groups go through the batched decode-layer engine (vox_engine_b16.hip: one launch per step for the 26 layers of both groups, cache
    // slices per slot through EngBParams::kv_row); wider steps, other geometries, VOX_BATCH_ENGINE=0 and the re-run after a hand-off timeout use the launch chains
    p.use_eng = allow_engine && !p.shared && have_jobs && !knob_str("VOX_BATCH_CONT_NO_ENGINE") && engb_prepare(m, 2);
    p.calib = !knob_str("VOX_BATCH_NO_CALIB"); p.no_fe_overlap = knob_str("VOX_BATCH_NO_FE_OVERLAP") != nullptr; p.no_graph = knob_str("VOX_BATCH_NO_GRAPH") != nullptr;
    p.verbose = knob_str("VOX_BATCH_VERBOSE") != nullptr; p.no_xcd = knob_str("VOX_ATTN_NO_XCD") != nullptr;
    if (const char* e = knob_str("VOX_BATCH_WIDE_MIN")) p.wide_min = std::max(2, std::min(5, atoi(e)));
    if (const char* e = knob_str("VOX_BATCH_WIDE_CHAINS")) p.wide_chains = std::max(2, std::min(4, atoi(e)));
    return p;
}
// The wide step serves the steps with >= wide_min active groups, 4 by default.  Measured (tools/wide_probe.py, 24 s clips, every slot busy; profiles/r06_wide_step.txt):
// 64 slots 3.26 ms per step against 3.55 on four launch chains, then forked, 48 slots 3.11 against 3.04.
// wide_split: a four-group step as TWO two-group wide chains instead of one four-group chain, run back to back on `s` like every chain of a step.  Measured with the two chains
// forked on two streams (round 6): a third of a wide step is dependency gaps between its ~236 launches (profiles/r06_corpus_sessions.txt), and the two chains filled
// each other's -- every weight is streamed twice, which a step at 0.7 TB/s can afford: 64-slot step 3.49 -> 3.29 ms (prefill included), corpus 4.54 -> 4.37 s, same
// ids (profiles/r06_wide_split.txt).  NOT on a shared GPU (vox_ctx_set_shared / sessions): there the other session already filled the gaps and four concurrent chains
// only contended (two sessions: 3.80 s without, 4.46 s with).  VOX_BATCH_NO_WIDE_SPLIT=1: one chain.
static void cont_policy_groups(ContPolicy& p, const vox_model* m, int G) {
    p.G = G;
    p.wide_ok = !p.no_wide && G >= p.wide_min && wide_geom_ok(m);
    p.wide_split = p.wide_ok && G >= 4 && p.wide_min <= 4 && !p.shared && !p.no_wide_split;
}
// What a step of `active` runs: the engine (groups ga, gb), nc wide chains of szc[j] groups from group 0, or (nc == 0) one launch chain per active group.  `bits`:
// the kernels it launches, for warm_forms (the dynamic-LDS limits are raised at a kernel's first launch on a device -- see cont_warm_forms).
enum : uint32_t { kChains = 1u, kEng1 = 2u, kEng2 = 4u, kWide2 = 8u };      // (kWide2 << (mt - 2): wide chains of mt = 2, 3, 4 groups)
struct StepForm {
    int n_act = 0, ga = -1, gb = -1, nc = 0, szc[4] = {0, 0, 0, 0}; uint32_t bits = 0;
    bool engine() const { return (bits & (kEng1 | kEng2)) != 0; }
    int report_slot() const { return (bits & kEng1) ? 1 : (bits & kEng2) ? 2 : nc == 1 ? 3 : nc > 1 ? 4 : 0; }      // cont_report: chains, engine1, engine2, wide, split
};
static StepForm form_of(const ContPolicy& p, uint32_t active) {
    StepForm f;
    for (int gi = 0; gi < p.G; gi++) if ((active >> gi) & 1u) { f.n_act++; if (f.ga < 0) f.ga = gi; else f.gb = gi; }
    if (p.use_eng && f.n_act <= 2) { f.bits = f.gb < 0 ? kEng1 : kEng2; return f; }
    if (p.wide_ok && f.n_act >= p.wide_min && active == (1u << f.n_act) - 1) {      // (active groups are a prefix: the slots are ordered by load)
        f.nc = p.wide_split && f.n_act >= 4 ? std::max(2, std::min(p.wide_chains, f.n_act / 2)) : 1;      // chains of >= 2 groups, sizes balanced, the larger ones first
        for (int j = 0; j < f.nc; j++) { f.szc[j] = f.n_act / f.nc + (j < f.n_act % f.nc ? 1 : 0); f.bits |= kWide2 << (f.szc[j] - 2); }
        return f;
    }
    f.bits = kChains; return f;
}
// The stacked encoder runs in chunks of <= CHUNK utterances, PACKED (encode_batch_dev: every utterance its own rows, no padding to the longest): chunk ci is utterances
// chunk0[ci] .. chunk0[ci + 1] - 1, its audio rows start aoff_c[ci] floats into the audio buffer and those of utterance i audio_off[i] floats; mel_max / smp_max: the
// largest chunk's log-mel floats / samples.  Host arithmetic only.
struct ChunkLayout { int n_chunks = 0; std::vector<int> chunk0; std::vector<size_t> aoff_c; std::vector<long> audio_off; size_t audio_floats = 0, mel_max = 0, smp_max = 0; };
static ChunkLayout chunk_layout(const vox_model* m, const std::vector<int>& T, const size_t* n_samples, int CHUNK) {
    const int n = (int)T.size(), R = m->cfg.reshape_factor, D = m->cfg.dec_dim;
    ChunkLayout z; z.n_chunks = (n + CHUNK - 1) / CHUNK;
    // full chunks first (measured on 81 utterances: 64 + 17 against 41 + 40 -- the packed encoder costs the same, 247 ms, the stacked prefill 57 instead of 66 ms)
    z.chunk0.assign(z.n_chunks + 1, 0);
    for (int ci = 0; ci < z.n_chunks; ci++) z.chunk0[ci + 1] = std::min(n, z.chunk0[ci] + CHUNK);
    z.aoff_c.resize(z.n_chunks); z.audio_off.resize(n);
    for (int ci = 0; ci < z.n_chunks; ci++) {
        const int c0 = z.chunk0[ci], nc = z.chunk0[ci + 1] - c0;
        z.aoff_c[ci] = z.audio_floats;
        size_t mf = 0, sf = 0; long rows = 0;
        for (int i = c0; i < c0 + nc; i++) { z.audio_off[i] = (long)(z.aoff_c[ci] + (size_t)(rows / R) * D); rows += enc_packed_rows_of(m, T[i]); mf += (size_t)128 * T[i]; sf += n_samples[i]; }
        z.audio_floats += (size_t)(rows / R) * D; z.mel_max = std::max(z.mel_max, mf); z.smp_max = std::max(z.smp_max, sf);
    }
    // slack behind the last utterance: a (never occurring, see test_audio_entry_points_never_reach_prefix_len_edge) S < 39 reads a row past its own
    z.audio_floats += (size_t)(VOX_PREFIX_TOKENS + 2) * D;
    return z;
}
// (an event where the set of active groups changes: the runs in between are what the planner's next session on this context is priced with)
struct StepSegments { int n[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, act[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, n_seg = 0; };
// One continuous session: the call's arguments, its plan (host only), its device buffers and its timers.  The pooled buffers go back to the pool when the session goes out
// of scope; `drain`, declared after them, empties the streams first.
struct ContSession {
    vox_model* m; vox_ctx* cx; hipStream_t s; MelTables mt;
    int n = 0; const float* const* samples = nullptr; const size_t* n_samples = nullptr; const float* const* unit_scale = nullptr; int32_t mem_kind = 0; const int* slot_of = nullptr;
    std::vector<int> S, T, len; int max_seq = 0, tstride = 0; size_t seq_stride = 0, layer_stride = 0;      // slice n of every layer: the scratch slice idle slots write to and read
    ContPolicy pol; ChunkLayout lay; SlotSchedule sch; double step_cost[9];
    bool fe_overlap = false; size_t mel_half = 1, smp_half = 1; int ncm = 0;      // front-end buffers: halves of the ping-pong, ncm = utterances of the largest chunk
    DevBuf b_audio, b_k, b_v, b_tok, b_posc, b_len, b_h0, b_aoff, b_px, b_xn, b_lg0, b_mel, b_scale, b_smp;
    DevBuf b_queue, b_sclip, b_sqpos, b_pos, b_kvrow, b_h, b_qkv, b_att, b_logits, b_ssq_e, b_planes; XfPlanes xfp; XfBufs xb{}; SlotStepParams sp{};      // the decode step's
    BatchTapCall tap; BatchRecordsCall rec; BatchDrain drain;
    double pre_ms = 0.0, enc_ms = 0.0, pf_ms = 0.0, t0 = 0.0, t1 = 0.0, capture_ms = 0.0; int replays = 0, n_captures = 0;
    int form_steps[5] = {0, 0, 0, 0, 0};      // VOX_BATCH_VERBOSE: decode steps on the launch chains, the one- / two-group engine, one wide chain, two or more wide chains
    explicit ContSession(vox_model* mm) : m(mm), cx(mm->ctx), s(mm->ctx->stream), drain{mm->ctx} {}
    // phase A's buffers and everything the host uploads once: prefix tokens, audio offsets, slot queues, the engine's layer table
    int32_t alloc() {
        const vox_model_cfg& c = m->cfg; const int D = c.dec_dim, V = c.vocab;
        HIPCHK(b_audio.alloc_pooled(cx, lay.audio_floats * 4)); HIPCHK(b_k.alloc_pooled(cx, layer_stride * c.dec_layers * 4)); HIPCHK(b_v.alloc_pooled(cx, layer_stride * c.dec_layers * 4));
        HIPCHK(b_tok.alloc_pooled(cx, (size_t)n * tstride * 4)); HIPCHK(b_posc.alloc_pooled(cx, (size_t)n * 4)); HIPCHK(b_len.alloc_pooled(cx, (size_t)n * 4));
        HIPCHK(b_h0.alloc_pooled(cx, (size_t)n * D * 4)); HIPCHK(b_aoff.alloc_pooled(cx, (size_t)n * sizeof(long)));
        ncm = std::min(n, pol.chunk);
        HIPCHK(b_px.alloc_pooled(cx, (size_t)ncm * VOX_PREFIX_TOKENS * D * 4)); HIPCHK(b_xn.alloc_pooled(cx, (size_t)ncm * D * 4)); HIPCHK(b_lg0.alloc_pooled(cx, (size_t)ncm * V * 4));
        // front-end buffers TWICE: chunk ci + 1's samples go up and its log-mel is computed on a second stream while chunk ci's encoder runs (VOX_BATCH_NO_FE_OVERLAP=1: one stream)
        // (not on a shared context: with two sessions uploading from two threads the second stream made each session's encoder stage 1.8 x longer under the HIP runtime that
        // PyTorch bundles -- bench.py: 3.82 -> 4.55 s for the two-session corpus -- while the stand-alone runtime did not care)
        fe_overlap = lay.n_chunks > 1 && !cx->shared && !pol.no_fe_overlap;
        const int halves = fe_overlap ? 2 : 1;
        mel_half = std::max<size_t>(lay.mel_max, 1); smp_half = std::max<size_t>(lay.smp_max, 1);
        HIPCHK(b_mel.alloc_pooled(cx, mel_half * 4 * halves)); HIPCHK(b_scale.alloc_pooled(cx, (size_t)ncm * 4 * halves));
        if (mem_kind == VOX_MEM_HOST) HIPCHK(b_smp.alloc_pooled(cx, smp_half * 4 * halves));
        if (fe_overlap) {
            if (!cx->fe_stream) HIPCHK(hipStreamCreateWithFlags(&cx->fe_stream, hipStreamNonBlocking));
            for (int k = 0; k < 2; k++) {
                if (!cx->ev_fe[k]) HIPCHK(hipEventCreateWithFlags(&cx->ev_fe[k], hipEventDisableTiming));
                if (!cx->ev_enc[k]) HIPCHK(hipEventCreateWithFlags(&cx->ev_enc[k], hipEventDisableTiming));
            }
        }
        HIPCHK(hipMemsetAsync(b_audio.p, 0, lay.audio_floats * 4, s)); HIPCHK(hipMemsetAsync(b_h0.p, 0, (size_t)n * D * 4, s));
        VOXCHK(upload_prefix(n, tstride, len, b_tok.as<int>(), b_posc.as<int>(), b_len.as<int>(), s));
        HIPCHK(hipMemcpyAsync(b_aoff.p, lay.audio_off.data(), (size_t)n * sizeof(long), hipMemcpyHostToDevice, s));
        const std::vector<int>& hq = sch.h_queue;      // (the slot queues too: no pageable copy may sit behind phase A)
        HIPCHK(b_queue.alloc_pooled(cx, hq.size() * 4)); HIPCHK(hipMemcpyAsync(b_queue.p, hq.data(), hq.size() * 4, hipMemcpyHostToDevice, s));
        std::vector<EngLayerTab> tab(c.dec_layers);      // the engine's layer table, one for every group: the layers' slabs (cache slices are picked per slot)
        dec_layer_tab(m, b_k.as<float>(), b_v.as<float>(), layer_stride, 0, tab.data());
        if (pol.use_eng) HIPCHK(hipMemcpyAsync(m->engb_tab[0], tab.data(), sizeof(EngLayerTab) * c.dec_layers, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));      // the host vectors go out of scope
        return VOX_OK;
    }
    // front-end of chunk cj (samples up, peak, log-mel) into half cj & 1 of the buffers, on stream sf; returns the chunk's mel pointers
    int32_t front_end(int cj, hipStream_t sf, std::vector<const float*>& d_mels) {
        const int c0 = lay.chunk0[cj], nc = lay.chunk0[cj + 1] - c0, half = fe_overlap ? (cj & 1) : 0;
        d_mels.assign(nc, nullptr);
        return front_end_units(mt, c0, nc, samples, n_samples, T.data(), unit_scale, mem_kind == VOX_MEM_HOST ? b_smp.as<float>() + (size_t)half * smp_half : nullptr,
                               b_mel.as<float>() + (size_t)half * mel_half, b_scale.as<float>() + (size_t)half * ncm, d_mels.data(), sf);
    }
    // the front-end overlap's event ping-pong, behind chunk ci's encoder on s: chunk ci + 1's front-end goes onto the second stream
    int32_t front_end_ahead(int ci, std::vector<const float*>& mels_next) {
        HIPCHK(hipEventRecord(cx->ev_enc[ci & 1], s));      // this chunk's encoder has read half ci & 1 of the front-end buffers
        if (ci + 1 < lay.n_chunks) {      // the next chunk's front-end: its half was last read by chunk ci - 1's encoder
            if (ci >= 1) HIPCHK(hipStreamWaitEvent(cx->fe_stream, cx->ev_enc[(ci + 1) & 1], 0));
            VOXCHK(front_end(ci + 1, cx->fe_stream, mels_next)); HIPCHK(hipEventRecord(cx->ev_fe[(ci + 1) & 1], cx->fe_stream));
        }
        return VOX_OK;
    }
    // ---- (A) one chunk: front-end, stacked encoder, stacked 38-token prefill, first token and first decode input h0 = audio[38] + embed(token) of its utterances
    int32_t stage_chunk(int ci, std::vector<const float*>& mels_cur, std::vector<const float*>& mels_next) {
        const int D = m->cfg.dec_dim, V = m->cfg.vocab;
        const int c0 = lay.chunk0[ci], nc = lay.chunk0[ci + 1] - c0;
        float* d_audio = b_audio.as<float>(); int* d_tok = b_tok.as<int>();
        const double ta = now_ms();
        if (!fe_overlap || ci == 0) { VOXCHK(front_end(ci, s, mels_cur)); HIPCHK(hipStreamSynchronize(s)); }
        else { mels_cur.swap(mels_next); HIPCHK(hipStreamWaitEvent(s, cx->ev_fe[ci & 1], 0)); }      // (issued under the previous chunk's encoder: front_end_ahead)
        const double tb = now_ms();
        std::vector<int> S4(nc); std::vector<long> aoff_rel(nc);
        VOXCHK(encode_batch_dev(m, nc, mels_cur.data(), T.data() + c0, d_audio + lay.aoff_c[ci], 0, S4.data(), aoff_rel.data()));
        for (int i = 0; i < nc; i++)
            ARGCHK(S4[i] == S[c0 + i] && (long)lay.aoff_c[ci] + aoff_rel[i] == lay.audio_off[c0 + i], "internal: sequence length / audio offset mismatch (%d vs %d)", S4[i], S[c0 + i]);
        if (fe_overlap) VOXCHK(front_end_ahead(ci, mels_next));
        HIPCHK(hipStreamSynchronize(s)); const double tc = now_ms();
        VOXCHK(prefill_first_logits(m, nc, d_tok + (size_t)c0 * tstride, tstride, d_audio, lay.audio_off.data() + c0, b_px.as<float>(), b_k.as<float>() + (size_t)c0 * seq_stride,
                                    b_v.as<float>() + (size_t)c0 * seq_stride, max_seq, layer_stride, seq_stride, b_xn.as<float>(), b_lg0.as<float>(), s));
        VOXCHK(tap.rows(b_lg0.as<float>(), nc, nullptr, c0, b_posc.as<int>() + c0, b_len.as<int>() + c0, s));
        VOXCHK(rec.rows(b_lg0.as<float>(), nc, nullptr, c0, b_posc.as<int>() + c0, b_len.as<int>() + c0, s));
        HIPCHK(launch_argmax_embed_batch(b_lg0.as<float>(), nc, V, d_tok + (size_t)c0 * tstride, tstride, b_posc.as<int>() + c0, b_len.as<int>() + c0, m->tok.w, d_audio, 0, D,
                                         b_h0.as<float>() + (size_t)c0 * D, s, nullptr, nullptr, nullptr, 0, 0, b_aoff.as<long>() + c0));
        // (the last chunk's prefill is not waited for here when a decode follows: the decode's buffers are set up and its graphs captured -- host work, ~6-10 ms per
        // distinct set of active groups -- while the GPU is still busy with it; the prefill timer closes behind that)
        const bool defer = ci == lay.n_chunks - 1 && sch.steps > 0;
        if (!defer) HIPCHK(hipStreamSynchronize(s));
        const double td = now_ms();
        pre_ms += tb - ta; enc_ms += tc - tb; pf_ms += td - tc;
        return VOX_OK;
    }
    // the decode's buffers: slot state, the step's rows and planes, the zeroed scratch cache slice, the wide step's planes scratch
    int32_t decode_alloc() {
        const vox_model_cfg& c = m->cfg;
        const int D = c.dec_dim, QD = c.dec_heads * c.dec_head_dim, W = QD + 2 * c.dec_kv_heads * c.dec_head_dim, V = c.vocab, G = sch.G, Sl = sch.Sl;
        HIPCHK(b_sclip.alloc_pooled(cx, (size_t)Sl * 4)); HIPCHK(b_sqpos.alloc_pooled(cx, (size_t)Sl * 4));
        HIPCHK(b_pos.alloc_pooled(cx, (size_t)Sl * 4)); HIPCHK(b_kvrow.alloc_pooled(cx, (size_t)Sl * 4)); HIPCHK(b_h.alloc_pooled(cx, (size_t)Sl * D * 4));
        HIPCHK(b_qkv.alloc_pooled(cx, (size_t)Sl * W * 4)); HIPCHK(b_att.alloc_pooled(cx, (size_t)Sl * QD * 4)); HIPCHK(b_logits.alloc_pooled(cx, (size_t)Sl * V * 4));
        VOXCHK(xfp.alloc(m, G, s, &xb));
        HIPCHK(hipMemsetAsync(b_h.p, 0, (size_t)Sl * D * 4, s)); HIPCHK(hipMemsetAsync(b_qkv.p, 0, (size_t)Sl * W * 4, s));
        // the scratch cache slice (index n of every layer): zeros, so that an idle slot's attention stays finite
        for (int l = 0; l < c.dec_layers; l++) {      // (one memset per layer: the pitch of a 2-D memset would be the layer stride -- tens of GB for a corpus-sized session)
            HIPCHK(hipMemsetAsync(b_k.as<float>() + (size_t)l * layer_stride + (size_t)n * seq_stride, 0, seq_stride * 4, s));
            HIPCHK(hipMemsetAsync(b_v.as<float>() + (size_t)l * layer_stride + (size_t)n * seq_stride, 0, seq_stride * 4, s));
        }
        if (pol.use_eng) HIPCHK(b_ssq_e.alloc_pooled(cx, (size_t)(256 + 16) * 16 * 4 * G));      // per group: the launch's 256 partial sums of squares + their fold
        xb.h = b_h.as<float>(); xb.qkv = b_qkv.as<float>(); xb.att = b_att.as<float>(); xb.logits = b_logits.as<float>();
        xb.k = b_k.as<float>(); xb.v = b_v.as<float>(); xb.layer_stride = layer_stride; xb.seq_stride = seq_stride; xb.max_seq = max_seq;
        xb.pos = b_pos.as<int>(); xb.kv_row = b_kvrow.as<int>(); xb.no_xcd_remap = pol.no_xcd; xb.ssq_e = b_ssq_e.as<float>();
        sp.logits = xb.logits; sp.vocab = V; sp.tokens = b_tok.as<int>(); sp.tok_stride = tstride; sp.clip_len = b_len.as<int>();
        sp.slot_clip = b_sclip.as<int>(); sp.slot_qpos = b_sqpos.as<int>(); sp.queue = b_queue.as<int>(); sp.q_stride = sch.q_stride;
        sp.pos = b_pos.as<int>(); sp.kv_row = b_kvrow.as<int>(); sp.n_clips = n; sp.first_pos = VOX_PREFIX_TOKENS; sp.tok = m->tok.w; sp.audio = b_audio.as<float>();
        sp.audio_off = b_aoff.as<long>(); sp.D = D;
        sp.h0 = b_h0.as<float>(); sp.h = xb.h; sp.xf = xb.xf1; sp.xf_w = m->dec[0].attn_norm; sp.ssq_out = xb.ssq;
        sp.xf_group_stride = xb.xf1_gs; sp.ssq_group_stride = (int)xb.ssq_gs;
        if (G > 4 && !pol.wide_split) return fail(VOX_ERR_INVALID, "internal: %d slot groups planned without the two-chain wide step", G);
        xb.planes_bytes = pol.wide_ok ? wide_planes_bytes(m, std::min(G, 4)) : 0;      // per chain
        if (pol.wide_ok) HIPCHK(b_planes.alloc_pooled(cx, xb.planes_bytes * (pol.wide_split ? pol.wide_chains : 1)));
        xb.planes = b_planes.p;
        return VOX_OK;
    }
    // ---- (C) the decode step over slots: every chain of the step's form back to back on `s`, then the argmax / next-input launch of all slots.  What the
    // graphs are captured from and the eager steps run.
    int32_t step(uint32_t active) {
        const StepForm f = form_of(pol, active);
        if (f.engine()) {
            if (f.gb < 0) HIPCHK(launch_decode_engine_b16(engb_params(m, xb, f.ga, 16, 0, 0, false), s));
            else HIPCHK(launch_decode_engine_b16x2(engb_params(m, xb, f.ga, 16, 0, 0, true), engb_params(m, xb, f.gb, 16, 0, 1, true), s));
            VOXCHK(engb_group_tail(m, xb, f.ga, 16, s));
            if (f.gb >= 0) VOXCHK(engb_group_tail(m, xb, f.gb, 16, s));
        } else if (f.nc > 0) {
            for (int j = 0, g0 = 0; j < f.nc; g0 += f.szc[j], j++) VOXCHK(xf_chain(m, xb, g0, 16, f.szc[j], j, true, 0, s));
        } else {
            for (int gi = 0; gi < sch.G; gi++)
                if ((active >> gi) & 1u) VOXCHK(xf_chain(m, xb, gi, 16, 0, 0, true, 0, s));
        }
        VOXCHK(tap.rows(xb.logits, sch.Sl, b_sclip.as<int>(), 0, xb.pos, nullptr, s));
        VOXCHK(rec.rows(xb.logits, sch.Sl, b_sclip.as<int>(), 0, xb.pos, nullptr, s));
        HIPCHK(launch_argmax_embed_slots(sp, sch.Sl, s));      // (retired groups' slots are idle: slot_clip < 0)
        return VOX_OK;
    }
    uint32_t eng_launches(uint32_t active) const { return form_of(pol, active).engine() ? 1u : 0u; }      // per step of `active`
    // The step's kernels raise their dynamic-LDS limits at their first launch on a device (hipFuncSetAttribute: not something to do inside a capture).  The chains a
    // step runs have different kernels (form_of's bits) and a plan may use several; the limits are per DEVICE, so the flags are the context's, not the process's (ADVICE
    // r5: a second vox_ctx on another GPU, or the launch chains after an engine-timeout re-run, met their first launch inside a capture; ADVICE r6: keyed by the number
    // of active groups, a shared call's four-group wide chain met its first launch inside a capture after an unshared call's two two-group chains).  A step that needs a
    // chain this context has not run yet takes ONE eager step on all-idle slots first (slot_clip -1: the argmax / next-input launch returns at once; zero rows against
    // the zeroed scratch slice; nothing of the session's state moves); every real step is then a graph replay.
    int32_t warm_forms() {
        const int Sl = sch.Sl;
        bool idle_set = false;
        for (int t = 0; t < sch.steps && !pol.no_graph; t++) {
            const uint32_t act = sch.active_at(t), f = form_of(pol, act).bits;
            if ((cx->warm_forms & f) == f) continue;
            if (!idle_set) {
                HIPCHK(hipMemsetAsync(b_sclip.p, 0xFF, (size_t)Sl * 4, s)); HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b_pos.p, VOX_PREFIX_TOKENS, Sl, s));
                HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b_kvrow.p, n, Sl, s)); idle_set = true;
            }
            VOXCHK(step(act)); m->engb_launches += eng_launches(act); cx->warm_forms |= f;
        }
        return VOX_OK;
    }
    // one graph per distinct set of active groups, captured NOW: the stream still holds the last chunk's prefill, the GPU is busy while the host records
    int32_t capture(StepGraphs& graphs) {
        auto one_step = [this](uint32_t active) { return step(active); };      // the single callable handed to StepGraphs::capture
        const double tg = now_ms();
        for (int t = 0; t < sch.steps; t++) {
            const uint32_t act = sch.active_at(t);
            if (graphs.find(act)) continue;
            hipGraphExec_t ge = nullptr;
            VOXCHK(graphs.capture(act, one_step, &ge));
            n_captures++;
        }
        capture_ms = now_ms() - tg;
        return VOX_OK;
    }
    // the decode loop: one graph replay (VOX_BATCH_NO_GRAPH: one eager step) per step of the schedule, a segment event wherever the set of active groups changes
    int32_t replay(StepGraphs& graphs, StepSegments& seg) {
        uint32_t last_act = 0;
        for (int t = 0; t < sch.steps; t++) {
            const uint32_t act = sch.active_at(t);
            if (pol.calib && !pol.no_graph && act != last_act && seg.n_seg < 9) {
                if (!cx->ev_seg[seg.n_seg]) HIPCHK(hipEventCreate(&cx->ev_seg[seg.n_seg]));
                HIPCHK(hipEventRecord(cx->ev_seg[seg.n_seg], s));
                seg.act[seg.n_seg] = __builtin_popcount(act); seg.n_seg++; last_act = act;
            }
            if (seg.n_seg > 0) seg.n[seg.n_seg - 1]++;
            form_steps[form_of(pol, act).report_slot()]++;
            m->engb_launches += eng_launches(act);
            if (pol.no_graph) { VOXCHK(step(act)); continue; }
            if (hipGraphLaunch(graphs.find(act), s) != hipSuccess) return fail(VOX_ERR_HIP, "hipGraphLaunch failed");
            replays++;
        }
        if (seg.n_seg > 0) { if (!cx->ev_seg[seg.n_seg]) HIPCHK(hipEventCreate(&cx->ev_seg[seg.n_seg])); HIPCHK(hipEventRecord(cx->ev_seg[seg.n_seg], s)); }
        return VOX_OK;
    }
    // the measured segment times into the context's step_ms_meas: runs of >= 8 steps only: shorter ones are mostly their first replay (a shared GPU: nothing is recorded)
    void fold_segments(const StepSegments& seg) {
        for (int k = 0; k < seg.n_seg && !cx->shared; k++) {
            float ms = 0.f;
            if (seg.n[k] >= 8 && seg.act[k] >= 1 && seg.act[k] <= kMaxGroups && hipEventElapsedTime(&ms, cx->ev_seg[k], cx->ev_seg[k + 1]) == hipSuccess && ms > 0.f) {
                double& mm = cx->step_ms_meas[pol.use_eng ? 0 : 1][seg.act[k]]; const double v = (double)ms / seg.n[k];
                mm = mm > 0.0 ? 0.7 * mm + 0.3 * v : v;
            } else (void)hipGetLastError();
        }
    }
    // ---- (B) + (C): the slot decode.  Set-up, warm-up and capture run on the host while the stream still holds the last chunk's prefill.
    int32_t decode() {
        VOXCHK(decode_alloc());
        StepGraphs graphs(s);
        VOXCHK(warm_forms());
        sp.init = 1; HIPCHK(launch_argmax_embed_slots(sp, sch.Sl, s)); sp.init = 0;      // every slot takes the first utterance of its queue
        if (!pol.no_graph) VOXCHK(capture(graphs));
        HIPCHK(hipStreamSynchronize(s));      // phase A (and the set-up behind it) is done: the prefill timer closes here, the decode timer starts
        { const double tn = now_ms(); pf_ms += tn - t1; t1 = tn; }
        StepSegments seg;
        VOXCHK(replay(graphs, seg));
        VOXCHK(engb_timeout_check(m, pol.use_eng ? 2 : 0, true, s));
        fold_segments(seg);
        return VOX_OK;
    }
    // VOX_BATCH_VERBOSE (tests/model_fixtures.py parses these lines)
    void report() const {
        const double* sc = step_cost; const int* fs = form_steps;
        fprintf(stderr, "[voxtral_hip] continuous batch: %d utterances, %d slots, %d steps (plan %.1f ms), front-end %.1f ms, encode %.1f ms (%d chunks), prefill %.1f ms "
                        "(%d graph captures, %.1f ms of host time, under the last chunk's), decode %.1f ms; step costs used %.2f / %.2f / %.2f / %.2f / %.2f / %.2f / %.2f / %.2f ms\n",
                n, sch.Sl, sch.steps, sch.plan.cost_ms, pre_ms, enc_ms, lay.n_chunks, pf_ms, n_captures, capture_ms, now_ms() - t1,
                sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], sc[7], sc[8]);
        fprintf(stderr, "[voxtral_hip] continuous batch step forms: chains %d, engine1 %d, engine2 %d, wide %d, split %d\n", fs[0], fs[1], fs[2], fs[3], fs[4]);
        std::string q = "[voxtral_hip] continuous batch slot plan (caller units per slot):";
        for (size_t sl = 0; sl < sch.plan.queue.size(); sl++) { q += sl ? " |" : " "; for (int u : sch.plan.queue[sl]) q += " " + std::to_string(slot_of[u]); }
        fprintf(stderr, "%s\n", q.c_str());
    }
};
// lengths -> plan -> buffers -> stage chunks -> decode -> copy out -> timings
static int32_t transcribe_continuous_impl(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const float* t_embed,
                                          int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind, const int* slot_of, bool allow_engine,
                                          const float* const* unit_scale = nullptr, const RecordsOut* rec_out = nullptr) {
    VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; const int PREFIX_LEN = VOX_PREFIX_TOKENS;
    ARGCHK(c.n_mels == 128, "the log-mel front-end produces 128 bins; model expects %d", c.n_mels);
    VOXCHK(vox_model_set_t_embed(m, t_embed));
    m->timings = vox_timings{};
    ContSession z(m); z.n = n; z.samples = samples; z.n_samples = n_samples; z.unit_scale = unit_scale; z.mem_kind = mem_kind; z.slot_of = slot_of;
    VOXCHK(ctx_mel_tables(z.cx, &z.mt));
    int Smax = 0;
    VOXCHK(batch_lengths(m, n, samples, n_samples, caps, slot_of, z.T, z.S, z.len, &Smax));
    z.max_seq = std::max((Smax + 63) / 64 * 64, 64); z.tstride = std::max(Smax, PREFIX_LEN) + 2;
    z.seq_stride = (size_t)c.dec_kv_heads * z.max_seq * c.dec_head_dim; z.layer_stride = (size_t)(n + 1) * z.seq_stride;
    // the plan (host only: lengths are known)
    std::vector<std::pair<int, int>> jobs;
    for (int i = 0; i < n; i++) if (z.len[i] > PREFIX_LEN + 1) jobs.emplace_back(z.len[i] - PREFIX_LEN - 1, i);
    z.pol = cont_policy(m, allow_engine, !jobs.empty());
    z.lay = chunk_layout(m, z.T, n_samples, z.pol.chunk);
    double base_tab[9]; for (int g2 = 0; g2 < 9; g2++) base_tab[g2] = (z.pol.use_eng ? kStepMsEng : kStepMs)[g2];
    // four groups as two two-group wide chains (cont_policy_groups): 3.12 -> 2.92 ms net of the prefill (measured with the chains forked)
    if (!z.pol.shared && !z.pol.no_wide_split) base_tab[4] = 2.95;
    step_costs(base_tab, z.cx->step_ms_meas[z.pol.use_eng ? 0 : 1], z.pol.calib, z.pol.shared, z.step_cost);
    z.sch = slot_schedule(jobs, z.pol.force_G, z.step_cost, z.pol.max_groups);
    cont_policy_groups(z.pol, m, z.sch.G);
    VOXCHK(z.tap.init(m, n, slot_of, z.s));
    VOXCHK(z.rec.init(m, n, z.S, rec_out, z.s));
    VOXCHK(z.alloc());
    z.t0 = now_ms();
    std::vector<const float*> mels_cur, mels_next;
    for (int ci = 0; ci < z.lay.n_chunks; ci++) VOXCHK(z.stage_chunk(ci, mels_cur, mels_next));
    z.t1 = now_ms();
    if (z.sch.steps > 0) VOXCHK(z.decode());
    int total = 0;
    VOXCHK(z.rec.download(z.s));
    VOXCHK(copy_out_ids(n, z.S, z.tstride, z.b_tok.as<int>(), out_ids, n_ids, &total, z.s));
    z.rec.scatter();
    m->timings.preprocess_ms = z.pre_ms; m->timings.encode_ms = z.enc_ms; m->timings.decode_ms = z.pf_ms + (now_ms() - z.t1); m->timings.total_ms = now_ms() - z.t0;
    m->timings.decode_tokens = total; m->timings.graph_replays = z.replays;
    if (z.pol.verbose) z.report();
    return VOX_OK;
}

// Entry point: rows are processed LONGEST FIRST (a stable sort of the caller's slots by sample count; sequence length is monotone in it), so that the
// 16-row groups of the decode loop retire last to first (see `step` above) -- results are per row and land in the caller's slot i whatever the internal order.
extern "C" int32_t vox_transcribe_batch(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const float* t_embed,
                                        int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind) {
    return vox_transcribe_batch_ex(m, n, samples, n_samples, nullptr, t_embed, out_ids, caps, n_ids, mem_kind);
}
// norm_group: the reference's CLI peak-normalises the FILE once (bin/transcribe.rs:207) and then splits it into chunks (:210-226); every chunk is an independent unit
// of work from there on (:231-265).  Units that name the same group >= 0 share ONE peak scale = 0.95 / max|x| over all of them (chunks tile their file, so that is the
// file's peak); group < 0: the unit is used as handed over (already normalised by the caller); norm_group == NULL: every unit normalises itself (un-chunked e2e-bench).
static int32_t transcribe_batch_one_session(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                            int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind_in, const RecordsOut* rec = nullptr);
// vox_model_set_sessions(m, S): batch calls with enough units run as S concurrent sessions on the model's GPU -- the calling thread on the model's own context, S - 1
// library threads on hidden contexts with replicas of the model (vox_model_replicate, device to device) -- see the header.  Units of one normalisation group stay in one
// session (the group's peak is reduced over the units of ONE session); LPT by sample count; every context involved is marked shared for the duration of the call.
static const int kMinUnitsPerSession = 128;      // below: one session (a small share is bound by its longest clip; 81 clips x0.82, 162 x0.86, 324 x1.16, 647 x1.20 with two sessions)
// A hidden session's stream on a hardware queue of its own: HIP spreads plain streams over a small pool of queues, and two sessions whose streams share one run one
// after the other (647-clip corpus, two sessions: 4.57 s against 3.80 s); a stream with a CU mask gets a queue of its own (every CU enabled).  Else: the plain stream.
static void ctx_own_queue(vox_ctx* c) {
    int ncu = 0; hipStream_t st = nullptr;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || ncu <= 0) { (void)hipGetLastError(); return; }
    std::vector<uint32_t> mask((ncu + 31) / 32, 0xFFFFFFFFu); if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1u;
    if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); return; }
    (void)hipStreamDestroy(c->stream); c->stream = st;
}
extern "C" int32_t vox_model_set_sessions(vox_model* m, int32_t sessions) {
    ARGCHK(m, "null model"); ARGCHK(sessions >= 1 && sessions <= 4, "sessions %d out of range (1..4)", sessions);
    if (sessions > 1 && (!m->is_q4 || m->manifest.empty())) return fail(VOX_ERR_UNSUPPORTED, "vox_model_set_sessions: Q4 (GGUF) models only");
    while ((int)m->twins.size() > sessions - 1) { vox_model* t = m->twins.back(); m->twins.pop_back(); vox_ctx* tc = t->ctx; model_release(t); (void)vox_ctx_destroy(tc); }
    while ((int)m->twins.size() < sessions - 1) {
        vox_ctx* tc = nullptr; VOXCHK(vox_ctx_create(m->ctx->device, &tc)); tc->shared = true; ctx_own_queue(tc);
        vox_model* t = nullptr; const int32_t r = vox_model_replicate(m, tc, &t);
        if (r != VOX_OK) { std::string e = vox_last_error(); (void)vox_ctx_destroy(tc); return fail(r, "%s", e.c_str()); }
        m->twins.push_back(t);
    }
    return ctx_bind(m->ctx);
}
static int32_t transcribe_batch_sessions(vox_model* m, int S, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                         int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind, const RecordsOut* rec) {
    const double t0 = now_ms();
    // groups of units (a normalisation group, or a unit on its own), heaviest first onto the least loaded session
    std::vector<std::vector<int>> members; { std::map<int32_t, int> by_id;
        for (int i = 0; i < n; i++) { if (norm_group && norm_group[i] >= 0) { auto it = by_id.find(norm_group[i]); if (it == by_id.end()) { by_id[norm_group[i]] = (int)members.size(); members.emplace_back(); it = by_id.find(norm_group[i]); } members[it->second].push_back(i); }
                                      else members.push_back({i}); } }
    std::vector<double> w(members.size(), 0.0); for (size_t g = 0; g < members.size(); g++) for (int i : members[g]) w[g] += (double)n_samples[i];
    std::vector<int> gi(members.size()); for (size_t g = 0; g < gi.size(); g++) gi[g] = (int)g;
    std::stable_sort(gi.begin(), gi.end(), [&](int a, int b) { return w[a] > w[b]; });
    std::vector<std::vector<int>> part(S); std::vector<double> load(S, 0.0);
    for (int g : gi) { int k = 0; for (int j = 1; j < S; j++) if (load[j] < load[k]) k = j; load[k] += w[g]; for (int i : members[g]) part[k].push_back(i); }
    for (auto& p : part) std::sort(p.begin(), p.end());
    struct Sub { std::vector<const float*> s; std::vector<size_t> ns; std::vector<int32_t> grp; std::vector<int32_t*> out; std::vector<int32_t> caps, nid; int32_t rc = VOX_OK; std::string err; vox_timings tm{};
                 std::vector<vox_token_score*> rs; std::vector<vox_token_alts*> ra; };      // (rs / ra: the session's units' record arrays of a scored call)
    std::vector<Sub> sub(S);
    for (int k = 0; k < S; k++) for (int i : part[k]) { Sub& u = sub[k]; u.s.push_back(samples[i]); u.ns.push_back(n_samples[i]); if (norm_group) u.grp.push_back(norm_group[i]); u.out.push_back(out_ids[i]); u.caps.push_back(caps[i]); u.nid.push_back(0);
                                                  if (rec && rec->scores) u.rs.push_back(rec->scores[i]); if (rec && rec->alts) u.ra.push_back(rec->alts[i]); }
    auto run = [&](int k) {
        Sub& u = sub[k]; vox_model* mk = k == 0 ? m : m->twins[(size_t)k - 1];
        if (u.s.empty()) return;
        const RecordsOut sub_rec{u.rs.empty() ? nullptr : u.rs.data(), u.ra.empty() ? nullptr : u.ra.data(), rec ? rec->k : 0};      // every session writes its own units' records
        u.rc = transcribe_batch_one_session(mk, (int32_t)u.s.size(), u.s.data(), u.ns.data(), norm_group ? u.grp.data() : nullptr, t_embed, u.out.data(), u.caps.data(), u.nid.data(), mem_kind,
                                            rec ? &sub_rec : nullptr);
        if (u.rc != VOX_OK) u.err = vox_last_error();      // (thread-local: read on the thread that failed)
        u.tm = mk->timings;
    };
    const bool was_shared = m->ctx->shared; m->ctx->shared = true;      // (the twins' contexts always are)
    std::vector<std::thread> th; std::vector<int> inline_k;      // (a session whose thread cannot be created runs on the calling thread, after its own)
    for (int k = 1; k < S; k++) { try { th.emplace_back(run, k); } catch (...) { inline_k.push_back(k); } }
    run(0);
    for (int k : inline_k) run(k);
    for (auto& t : th) t.join();
    m->ctx->shared = was_shared;
    (void)ctx_bind(m->ctx);
    for (int k = 0; k < S; k++) if (sub[k].rc != VOX_OK) return fail(sub[k].rc, "session %d of %d: %s", k, S, sub[k].err.c_str());
    int total = 0;
    for (int k = 0; k < S; k++) for (size_t j = 0; j < part[k].size(); j++) { n_ids[part[k][j]] = sub[k].nid[j]; total += sub[k].nid[j]; }
    // stage times: the longest session's (they overlap); tokens and replays: the sum; total: this call's wall time
    vox_timings tm = sub[0].tm;
    for (int k = 1; k < S; k++) { tm.preprocess_ms = std::max(tm.preprocess_ms, sub[k].tm.preprocess_ms); tm.encode_ms = std::max(tm.encode_ms, sub[k].tm.encode_ms); tm.decode_ms = std::max(tm.decode_ms, sub[k].tm.decode_ms);
                                  tm.graph_replays += sub[k].tm.graph_replays; }
    tm.decode_tokens = total; tm.total_ms = now_ms() - t0; m->timings = tm;
    return VOX_OK;
}
static int32_t transcribe_batch_entry(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                      int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind_in, const RecordsOut* rec);
extern "C" int32_t vox_transcribe_batch_ex(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                           int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind_in) {
    return transcribe_batch_entry(m, n, samples_in, n_samples, norm_group, t_embed, out_ids, caps, n_ids, mem_kind_in, nullptr);
}
// the same call with a record per id (see the header): every argument is checked here, before a device is touched
extern "C" int32_t vox_transcribe_batch_scored(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                               int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, vox_token_score* const* scores, vox_token_alts* const* alts,
                                               int32_t k, int32_t mem_kind) {
    ARGCHK(m, "null model"); ARGCHK(samples && n_samples && t_embed && out_ids, "null argument"); ARGCHK(caps, "null caps"); ARGCHK(n_ids, "null n_ids");
    ARGCHK(n > 0 && n <= 4096, "batch size %d out of range (1..4096)", n);
    VOXCHK(records_args_check(scores, alts, k));
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    for (int i = 0; i < n; i++) {
        ARGCHK(out_ids[i] || caps[i] <= 0, "null out_ids[%d]", i);
        ARGCHK(!scores || scores[i] || caps[i] <= 0, "null scores[%d]", i); ARGCHK(!alts || alts[i] || caps[i] <= 0, "null alts[%d]", i);
    }
    const RecordsOut rec{scores, alts, k};
    return transcribe_batch_entry(m, n, samples, n_samples, norm_group, t_embed, out_ids, caps, n_ids, mem_kind, &rec);
}
static int32_t transcribe_batch_entry(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                      int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind_in, const RecordsOut* rec) {
    ARGCHK(m, "null model");
    const bool tapped = m->tap.armed; m->tap.armed = false;      // an armed tap is consumed by this call, whatever its outcome
    ARGCHK(samples_in && n_samples && t_embed && out_ids && caps && n_ids, "null argument"); ARGCHK(n > 0 && n <= 4096, "batch size %d out of range (1..4096)", n);
    if (tapped) {
        for (int u : m->tap.units) ARGCHK(u < n, "tapped unit %d out of range (batch of %d)", u, n);
        VOXCHK(ctx_bind(m->ctx));
        const size_t bytes = m->tap.units.size() * (size_t)m->tap.max_rows * m->cfg.vocab * 4;
        HIPCHK(hipMalloc((void**)&m->tap.out, bytes)); HIPCHK(hipMalloc((void**)&m->tap.rows, m->tap.units.size() * 4));
        HIPCHK(hipMemset(m->tap.out, 0, bytes)); HIPCHK(hipMemset(m->tap.rows, 0, m->tap.units.size() * 4));
    }
    if (!m->twins.empty() && !knob_str("VOX_BATCH_ONE_SESSION")) {
        const int S = std::min((int)m->twins.size() + 1, n / kMinUnitsPerSession);
        if (S > 1 && tapped) return fail(VOX_ERR_UNSUPPORTED, "the batch logits tap covers one session: this call would run as %d (vox_model_set_sessions)", S);
        if (S > 1) { for (int i = 0; i < n; i++) ARGCHK(samples_in[i] && n_samples[i] > 0, "empty audio in batch slot %d", i);
                     return transcribe_batch_sessions(m, S, n, samples_in, n_samples, norm_group, t_embed, out_ids, caps, n_ids, mem_kind_in, rec); }
    }
    m->tap.on = tapped;
    const int32_t r = transcribe_batch_one_session(m, n, samples_in, n_samples, norm_group, t_embed, out_ids, caps, n_ids, mem_kind_in, rec);
    m->tap.on = false; m->tap.ready = tapped && r == VOX_OK;
    return r;
}
// the group peaks of a vox_transcribe_batch_ex call: pooled buffers, per unit (caller's order) its device samples (host samples only) and its device scale cell
struct GroupScales { DevBuf b_all, b_gmax, b_ugrp, b_uscale; std::vector<const float*> dev_s, scale_of; };
// every unit's scale = 0.95 / the peak of its norm_group (1: a silent group, a unit with a negative group), reduced on the device; host samples go up once, here, each
// unit 16-byte aligned (g.dev_s).  Synchronises the stream once: the scales are ready for every session of the call.
static int32_t group_peak_scales(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, int32_t mem_kind_in, GroupScales& g) {
    const float* const* samples = samples_in;
    VOXCHK(ctx_bind(m->ctx)); vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    std::vector<int> ug(n); std::vector<int32_t> ids; ids.reserve(n);      // dense group index per unit
    {
        std::vector<int32_t> uniq; for (int i = 0; i < n; i++) if (norm_group[i] >= 0) uniq.push_back(norm_group[i]);
        std::sort(uniq.begin(), uniq.end()); uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        for (int i = 0; i < n; i++) ug[i] = norm_group[i] < 0 ? -1 : (int)(std::lower_bound(uniq.begin(), uniq.end(), norm_group[i]) - uniq.begin());
        ids = uniq;
    }
    for (int i = 0; i < n; i++) ARGCHK(samples_in[i] && n_samples[i] > 0, "empty audio in batch slot %d", i);
    if (mem_kind_in == VOX_MEM_HOST) {      // the peaks are reduced on the device: the whole call's samples go up once, here (4 B per sample: 0.4 GB for a 647-clip corpus)
        size_t tot = 0; for (int i = 0; i < n; i++) tot += (n_samples[i] + 3) & ~(size_t)3;
        HIPCHK(g.b_all.alloc_pooled(cx, tot * 4));
        g.dev_s.resize(n); size_t o = 0;
        for (int i = 0; i < n; i++) { float* d = g.b_all.as<float>() + o; o += (n_samples[i] + 3) & ~(size_t)3; HIPCHK(hipMemcpyAsync(d, samples_in[i], n_samples[i] * 4, hipMemcpyHostToDevice, s)); g.dev_s[i] = d; }
        samples = g.dev_s.data();
    }
    const size_t ng = std::max<size_t>(ids.size(), 1);
    HIPCHK(g.b_gmax.alloc_pooled(cx, ng * 4)); HIPCHK(g.b_ugrp.alloc_pooled(cx, (size_t)n * 4)); HIPCHK(g.b_uscale.alloc_pooled(cx, (size_t)n * 4));
    HIPCHK(hipMemsetAsync(g.b_gmax.p, 0, ng * 4, s)); HIPCHK(hipMemcpyAsync(g.b_ugrp.p, ug.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    for (int i = 0; i < n; i++) if (ug[i] >= 0) HIPCHK(launch_absmax_group(samples[i], (long)n_samples[i], g.b_gmax.as<unsigned>() + ug[i], s));
    HIPCHK(launch_group_scale(g.b_gmax.as<unsigned>(), g.b_ugrp.as<int>(), n, 0.95f, g.b_uscale.as<float>(), s));
    HIPCHK(hipStreamSynchronize(s));      // `ug` (pageable) goes out of scope; the scales are ready for every session below
    g.scale_of.resize(n); for (int i = 0; i < n; i++) g.scale_of[i] = g.b_uscale.as<float>() + i;
    return VOX_OK;
}
static int32_t transcribe_batch_one_session(vox_model* m, int32_t n, const float* const* samples_in, const size_t* n_samples, const int32_t* norm_group, const float* t_embed,
                                            int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind_in, const RecordsOut* rec) {
    const float* const* samples = samples_in; int32_t mem_kind = mem_kind_in;
    GroupScales gs;      // (declared before everything that launches on its buffers; the impls drain the streams before they return)
    if (norm_group) {
        VOXCHK(group_peak_scales(m, n, samples_in, n_samples, norm_group, mem_kind_in, gs));
        if (!gs.dev_s.empty()) { samples = gs.dev_s.data(); mem_kind = VOX_MEM_DEVICE; }
    }
    const std::vector<const float*>& scale_of = gs.scale_of;
    struct DrainAll { vox_model* m; bool on; ~DrainAll() { if (on) { (void)hipStreamSynchronize(m->ctx->stream); } } } drain_all{m, norm_group != nullptr};
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    if (n > 16 && !knob_str("VOX_BATCH_NO_SORT"))
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_samples[a] > n_samples[b]; });
    std::vector<const float*> p_s(n), p_sc(n, nullptr); std::vector<size_t> p_n(n); std::vector<int32_t*> p_o(n); std::vector<int32_t> p_c(n), p_k(n, 0);
    for (int i = 0; i < n; i++) { const int o = order[i]; p_s[i] = samples[o]; p_n[i] = n_samples[o]; p_o[i] = out_ids[o]; p_c[i] = caps[o]; if (norm_group) p_sc[i] = scale_of[o]; }
    std::vector<vox_token_score*> p_rs; std::vector<vox_token_alts*> p_ra;      // the record arrays in the same order
    if (rec && rec->scores) { p_rs.resize(n); for (int i = 0; i < n; i++) p_rs[i] = rec->scores[order[i]]; }
    if (rec && rec->alts) { p_ra.resize(n); for (int i = 0; i < n; i++) p_ra[i] = rec->alts[order[i]]; }
    const float* const* usc = norm_group ? p_sc.data() : nullptr;
    // <= 16 rows: one group (the batched decode-layer engine).  Wider: continuous batching over slots, in sessions whose resident K / V stays under 64 GB (212 992 B per
    // position and utterance: 54 MB at 256 positions -> 1 174 utterances; every session pays its own tail and graph captures, so the 647-clip corpus is ONE session);
    // VOX_BATCH_NO_CONTINUOUS=1 (or a geometry / checkpoint the XF step does not cover): lock-step batches of <= 64 rows.
    const bool cont = n > 16 && batch_xf_ok(m) && !knob_str("VOX_BATCH_NO_CONTINUOUS");
    int part_max = 64;
    if (cont) {
        const vox_model_cfg& c = m->cfg; vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
        const size_t left = pad_left(&pc), total = left + p_n[0] + pad_right(&pc, p_n[0] + left);      // the longest utterance (rows are sorted) sets max_seq
        const int Smax = conv_len(conv_len((int)(total / 160))) / c.reshape_factor, max_seq = std::max((Smax + 63) / 64 * 64, 64);
        // resident per utterance: its K / V slices + its audio rows ([max_seq][dec_dim] f32) + token / input rows; beside them ONE encoder / prefill stack of <= 64 utterances
        // lives at a time (packed encoder workspace ~ 80 MB per 30 s utterance: activations, q|k|v, FFN rows in f32 + XF planes; logits of the chunk): a fixed reserve
        const double per_clip = 2.0 * c.dec_layers * (double)c.dec_kv_heads * max_seq * c.dec_head_dim * 4.0 + (double)max_seq * c.dec_dim * 4.0 + (double)p_n[0] * 4.0;
        const double reserve = 64.0 * 80e6 + 64.0 * (double)c.vocab * 4.0 + 1e9;
        double budget = 64e9;
        {   // ... and under half of what the device has free right now (a shared GPU, other models resident): the pooled buffers of earlier calls count as free for this purpose
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) { size_t pooled = 0; for (const auto& e : m->ctx->pool) if (!e.used) pooled += e.cap; budget = std::min(budget, 0.5 * (double)(free_b + pooled)); }
            else (void)hipGetLastError();
        }
        part_max = (int)std::max(17.0, std::min(4096.0, (budget - std::min(reserve, 0.5 * budget)) / per_clip));
        if (const char* e = knob_str("VOX_BATCH_SESSION_MAX")) part_max = std::max(17, atoi(e));      // measurement knob
    }
    const int n_parts = (n + part_max - 1) / part_max;
    m->batch_sessions = 0; vox_timings acc{}; int32_t r = VOX_OK;
    for (int pi = 0, a = 0; pi < n_parts && r == VOX_OK; pi++) {
        const int b = a + (n - a) / (n_parts - pi);      // equal contiguous parts of the sorted order
        const int np = b - a;
        const RecordsOut part_rec{p_rs.empty() ? nullptr : p_rs.data() + a, p_ra.empty() ? nullptr : p_ra.data() + a, rec ? rec->k : 0};
        r = retry_on_launches([&](bool engine) {
            return (cont ? transcribe_continuous_impl : transcribe_batch_impl)(m, np, p_s.data() + a, p_n.data() + a, t_embed, p_o.data() + a, p_c.data() + a, p_k.data() + a, mem_kind,
                                                                               order.data() + a, engine, usc ? usc + a : nullptr, rec ? &part_rec : nullptr);
        });
        acc.preprocess_ms += m->timings.preprocess_ms; acc.encode_ms += m->timings.encode_ms; acc.decode_ms += m->timings.decode_ms; acc.total_ms += m->timings.total_ms;
        acc.decode_tokens += m->timings.decode_tokens; acc.graph_replays += m->timings.graph_replays;
        m->batch_sessions++; a = b;
    }
    if (r == VOX_OK) { m->timings = acc; for (int i = 0; i < n; i++) n_ids[order[i]] = p_k[i]; }
    return r;
}

// ------------------------------------------------------------------------------------------------
// Piecewise decoder surface: the loop of bin/e2e_bench.rs:179-224 and web/bindings.rs:357-424 drives decode as
//   embed_tokens_from_ids -> (+ audio row) -> forward_hidden_with_cache -> lm_head -> argmax -> scalar read-back
// on device-resident tensors.  The `_ex` entries take mem_kind like the rest of the header (VOX_MEM_DEVICE: nothing is copied, nothing is synchronised), use
// model-owned workspaces (no hipMalloc / hipFree per call), and a single-row forward_hidden_with_cache on an engine-eligible cache is ONE launch of the decode
// engine -- which computes that row's lm_head as well; lm_head / lm_head_argmax on the hidden buffer it returned find the logits already there.
// ------------------------------------------------------------------------------------------------
static int32_t pw_ids_dev(vox_model* m, const int32_t* ids, int n) {      // host token ids -> m->pw_ids (range-checked)
    const vox_model_cfg& c = m->cfg;
    for (int i = 0; i < n; i++) ARGCHK(ids[i] >= 0 && ids[i] < c.vocab, "token id %d out of range", ids[i]);
    if (m->pw_ids_cap < n) {
        if (m->pw_ids) HIPCHK(hipFree(m->pw_ids));
        m->pw_ids = nullptr; m->pw_ids_cap = 0;
        const int cap = std::max(n, 64); HIPCHK(hipMalloc((void**)&m->pw_ids, (size_t)cap * 4)); m->pw_ids_cap = cap;
    }
    HIPCHK(hipMemcpyAsync(m->pw_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, m->ctx->stream));
    return VOX_OK;
}
// is the decode engine usable for ONE row against the caller's cache?  Binds the piecewise table to that cache on first use.
static bool pw_engine_ready(vox_model* m, vox_cache* kc) {
    if (kc->len >= kc->max_seq || !engine_bind(m, m->eng_pw, kc)) return false;
    if (m->pw_zero) return true;      // the launch's position word: position = 0 + cache length
    if (hipMalloc((void**)&m->pw_zero, 4) == hipSuccess && hipMemsetAsync(m->pw_zero, 0, 4, m->ctx->stream) == hipSuccess) return true;
    (void)hipGetLastError(); if (m->pw_zero) (void)hipFree(m->pw_zero); m->pw_zero = nullptr; return false;
}
// after a stream synchronisation that covered a copy of the engine's error word into eng_pw.err_word: a hand-off timeout fails the call loudly (the cache row of that step is
// rewritten when the caller repeats it), counts a strike and re-arms the engine; three strikes switch it off for the model
// (the error word reaches the host through a pinned buffer refreshed asynchronously behind every engine launch: a caller that stays on the device-resident entries
// -- whose only synchronisation is vox_argmax_rows on the CONTEXT -- still gets the failure at its next decoder call, not silently wrong logits)
static int32_t pw_engine_verdict(vox_model* m) {
    if (!m->eng_pw.err_word) return VOX_OK;
    const unsigned e = *(volatile unsigned*)m->eng_pw.err_word;
    if (!e) return VOX_OK;
    m->eng_pw.err_word[0] = 0u; m->pw_eng_used = false;
    m->pw_memo = false; m->pw_verdict_failed = true;
    // take back every row that is not known to be good: the failed step's, and whatever was appended behind it before the failure was seen
    int len_now = -1;
    if (m->pw_pend_rows > 0 && m->pw_pend_cache && cache_alive(m->pw_pend_cache, m->pw_pend_gen)) { m->pw_pend_cache->len = std::max(m->pw_pend_cache->len - m->pw_pend_rows, 0); len_now = m->pw_pend_cache->len; }
    m->pw_pend_rows = 0; m->pw_pend_cache = nullptr; if (m->ctx->pw_model == m) m->ctx->pw_model = nullptr;
    VOXCHK(engine_strike(m));
    return fail(VOX_ERR_HIP, "decode engine: %s: the GPU is shared; the KV cache is back at length %d -- repeat the step%s", engine_timeout_text(e, m->eng_strikes).c_str(),
                len_now, m->eng_strikes >= 3 ? " (the engine is now switched off, the per-operator launches serve it)" : "");
}
// behind a synchronisation of the stream: the pinned error word of every engine launch enqueued so far has landed -- read the verdict; clean: every pending row is verified
namespace vox_host {
int32_t pw_after_sync(vox_model* m) {
    m->pw_eng_used = false;
    const int32_t r = pw_engine_verdict(m);
    if (r == VOX_OK) { m->pw_pend_rows = 0; m->pw_pend_cache = nullptr; if (m->ctx->pw_model == m) m->ctx->pw_model = nullptr; }
    return r;
}
int32_t pw_sync(vox_model* m) {      // synchronise the stream (the pinned error word of an outstanding engine launch lands with the same wait), then the verdict
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    return pw_after_sync(m);
}
}  // namespace vox_host
// rows appended to `kc` by a step that cannot be verified yet (an engine launch, or anything behind one): remembered until the next synchronisation
static int32_t pw_note_pending(vox_model* m, vox_cache* kc, int rows) {
    if (m->pw_pend_rows > 0 && (m->pw_pend_cache != kc || m->pw_pend_gen != kc->gen)) VOXCHK(pw_sync(m));      // another cache's steps are outstanding: settle them first
    m->pw_pend_cache = kc; m->pw_pend_gen = kc->gen; m->pw_pend_rows += rows; m->ctx->pw_model = m;
    return VOX_OK;
}

extern "C" int32_t vox_embed_tokens_from_ids_ex(vox_model* m, const int32_t* ids, int32_t n, float* out, int32_t mem_kind) {
    ARGCHK(m && ids && out && n > 0, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    VOXCHK(pw_ids_dev(m, ids, n));
    float* dx = out;
    if (mem_kind != VOX_MEM_DEVICE) { VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)n * c.dec_dim)); dx = m->pw_x; }
    HIPCHK(launch_embed(m->tok.w, m->pw_ids, n, nullptr, c.dec_dim, nullptr, 0, 0, dx, s));
    if (mem_kind != VOX_MEM_DEVICE) { HIPCHK(hipMemcpyAsync(out, dx, (size_t)n * c.dec_dim * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
    return VOX_OK;
}
extern "C" int32_t vox_embed_tokens_from_ids(vox_model* m, const int32_t* ids, int32_t n, float* out) { return vox_embed_tokens_from_ids_ex(m, ids, n, out, VOX_MEM_HOST); }

// `audio_pos + text_embed` (e2e_bench.rs:212, model.rs:902,946) on the context's stream
extern "C" int32_t vox_tensor_add(vox_ctx* c, const float* a, const float* b, size_t n, float* out, int32_t mem_kind) {
    ARGCHK(c && a && b && out && n > 0, "bad argument"); VOXCHK(ctx_bind(c));
    if (mem_kind == VOX_MEM_DEVICE) { HIPCHK(launch_add_rows(a, b, out, (long)n, c->stream)); return VOX_OK; }
    for (size_t i = 0; i < n; i++) out[i] = a[i] + b[i];
    return VOX_OK;
}

extern "C" int32_t vox_forward_hidden_with_cache_ex(vox_model* m, const float* x, int32_t M, const float* t_embed, vox_cache* kc, float* out, const float** hidden_ws,
                                                    int32_t mem_kind) {
    ARGCHK(m && x && t_embed && kc && (out || hidden_ws) && M > 0, "bad argument"); ARGCHK(kc->m == m && kc->kind == 0, "cache belongs to another model or is an encoder cache"); VOXCHK(ctx_bind(m->ctx));
    ARGCHK(mem_kind == VOX_MEM_DEVICE || out, "a host result needs an output buffer");
    VOXCHK(pw_engine_verdict(m));      // a hand-off timeout of an EARLIER engine step the caller has synchronised past since (free: a pinned host word)
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream; const int D = c.dec_dim;
    ARGCHK(kc->len + M <= kc->max_seq, "KV cache overflow: %d + %d > %d", kc->len, M, kc->max_seq);
    VOXCHK(vox_model_set_t_embed(m, t_embed));
    m->pw_memo = false;
    // the residual stream is updated in place by the layer stack: always work on the model's copy of the input rows
    VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)M * D)); VOXCHK(ensure(&m->pw_hidden, &m->pw_hidden_cap, (size_t)M * D));
    const bool eng = M == 1 && pw_engine_ready(m, kc);
    if (eng) VOXCHK(ensure(&m->pw_logits, &m->pw_logits_cap, (size_t)c.vocab));
    const float* xin = x;
    if (mem_kind != VOX_MEM_DEVICE) { HIPCHK(hipMemcpyAsync(m->pw_x, x, (size_t)M * D * 4, hipMemcpyHostToDevice, s)); xin = m->pw_x; }
    if (eng) {      // one launch: 26 layers against the caller's cache + final norm + lm_head (logits + argmax partials)
        VOXCHK(engine_take_serials(m, 1, s));
        const EngParams ep = engine_params(m, m->eng_pw, kc, xin, m->pw_zero, kc->len, m->pw_logits);
        HIPCHK(launch_decode_engine(ep, s));
        HIPCHK(launch_eng_hidden(ep, m->pw_hidden, s));
        VOXCHK(engine_err_enqueue(m, m->eng_pw.err_word, s));      // pinned destination: truly asynchronous
        m->pw_memo = true; m->pw_eng_used = true;
    } else {
        if (xin != m->pw_x) HIPCHK(hipMemcpyAsync(m->pw_x, xin, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
        if (M == 1) { VOXCHK(wo_acc_clear(m, s)); VOXCHK(decoder_step_dev(m, m->pw_x, kc, nullptr, kc->len)); }
        else VOXCHK(decoder_prefill_dev(m, m->pw_x, M, kc, kc->len));
        HIPCHK(launch_rms_norm(m->pw_x, D, M, D, m->dec_norm, nullptr, c.norm_eps, m->pw_hidden, D, s));   // model.rs:676
    }
    const int len0 = kc->len;
    if (eng || m->pw_pend_rows > 0) VOXCHK(pw_note_pending(m, kc, M));      // (before the length moves: a failure found by the settling sync leaves the cache as it was)
    kc->len += M;
    if (hidden_ws) *hidden_ws = m->pw_hidden;
    if (out && out != m->pw_hidden) HIPCHK(hipMemcpyAsync(out, m->pw_hidden, (size_t)M * D * 4, mem_kind == VOX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (mem_kind != VOX_MEM_DEVICE) {
        const int32_t r = pw_sync(m);
        if (r != VOX_OK) { kc->len = std::min(kc->len, len0); return r; }      // (a hand-off timeout has already taken its pending rows back: never below that)
    }
    return VOX_OK;
}
extern "C" int32_t vox_forward_hidden_with_cache(vox_model* m, const float* x, int32_t M, const float* t_embed, vox_cache* kc, float* out) {
    return vox_forward_hidden_with_cache_ex(m, x, M, t_embed, kc, out, nullptr, VOX_MEM_HOST);
}

// does `hidden` name the row whose logits the engine launch of the last forward_hidden_with_cache already produced?
static bool pw_memo_hit(const vox_model* m, const float* hidden, int M, int mem_kind) { return m->pw_memo && M == 1 && mem_kind == VOX_MEM_DEVICE && hidden == m->pw_hidden; }

extern "C" int32_t vox_lm_head_ex(vox_model* m, const float* hidden, int32_t M, float* logits, int32_t mem_kind) {
    ARGCHK(m && hidden && logits && M > 0, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (pw_memo_hit(m, hidden, M, mem_kind)) {      // computed by the engine launch that produced `hidden`
        if (logits != m->pw_logits) HIPCHK(hipMemcpyAsync(logits, m->pw_logits, (size_t)c.vocab * 4, hipMemcpyDeviceToDevice, s));
        return VOX_OK;
    }
    const float* hx = hidden; float* ly = logits;
    if (mem_kind != VOX_MEM_DEVICE) {
        // (a host caller that passes back the rows forward_hidden_with_cache handed out gets the same engine-made logits: compare the bytes, 12 KB)
        if (m->pw_memo && M == 1) {
            std::vector<float> hh(c.dec_dim); HIPCHK(hipMemcpyAsync(hh.data(), m->pw_hidden, (size_t)c.dec_dim * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
            if (!std::memcmp(hh.data(), hidden, (size_t)c.dec_dim * 4)) {
                HIPCHK(hipMemcpyAsync(logits, m->pw_logits, (size_t)c.vocab * 4, hipMemcpyDeviceToHost, s));
                return pw_sync(m);
            }
        }
        VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)M * c.dec_dim)); VOXCHK(ensure(&m->pw_logits, &m->pw_logits_cap, (size_t)M * c.vocab));
        m->pw_memo = false;      // pw_logits is about to be overwritten
        HIPCHK(hipMemcpyAsync(m->pw_x, hidden, (size_t)M * c.dec_dim * 4, hipMemcpyHostToDevice, s)); hx = m->pw_x; ly = m->pw_logits;
    }
    VOXCHK(q4_linear_dev(m->ctx, m->tok.w, nullptr, hx, c.dec_dim, M, ly, c.vocab));
    if (mem_kind != VOX_MEM_DEVICE) { HIPCHK(hipMemcpyAsync(logits, ly, (size_t)M * c.vocab * 4, hipMemcpyDeviceToHost, s)); return pw_sync(m); }
    return VOX_OK;
}
extern "C" int32_t vox_lm_head(vox_model* m, const float* hidden, int32_t M, float* logits) { return vox_lm_head_ex(m, hidden, M, logits, VOX_MEM_HOST); }

// the device rule on a host row (vox_kernels.h, above launch_argmax_final): NaN never wins, lowest index on ties, 0 when nothing wins
static int argmax_row_host(const float* row, int V) {
    float v = -INFINITY; int b = 0x7fffffff;
    for (int i = 0; i < V; i++) if (row[i] > v || (row[i] == v && i < b)) { v = row[i]; b = i; }
    return b == 0x7fffffff ? 0 : b;
}
// `logits.argmax(2)` + the scalar read-back (e2e_bench.rs:219-220): ids always host; synchronises the stream
extern "C" int32_t vox_argmax_rows(vox_ctx* c, const float* logits, int32_t M, int32_t V, int32_t* ids, int32_t mem_kind) {
    ARGCHK(c && logits && ids && M > 0 && V > 0, "bad argument"); VOXCHK(ctx_bind(c));
    if (mem_kind != VOX_MEM_DEVICE) {
        for (int r = 0; r < M; r++) ids[r] = argmax_row_host(logits + (size_t)r * V, V);
        return VOX_OK;
    }
    DevBuf di; HIPCHK(di.alloc_pooled(c, (size_t)M * 4));
    HIPCHK(launch_argmax_rows(logits, M, V, di.as<int>(), c->stream));
    HIPCHK(hipMemcpyAsync(ids, di.p, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    if (c->pw_model) return pw_after_sync(c->pw_model);      // the reference loop's ONLY synchronisation (e2e_bench.rs:219-220): an engine hand-off timeout of this very step is reported here, with the cache rolled back
    return VOX_OK;
}

// vox_argmax_rows' companion: a vox_token_score per row (launch_score_rows: the kernel the live sessions' scores come from).  Every check before the context is
// bound; host logits are uploaded -- there is one implementation, the device's.  out host; synchronises.
static_assert(sizeof(vox_token_score) == 16 && sizeof(TokenScore) == sizeof(vox_token_score), "vox_token_score is TokenScore");
extern "C" int32_t vox_score_rows(vox_ctx* c, const float* logits, int32_t M, int32_t V, const int32_t* ids, vox_token_score* out, int32_t mem_kind) {
    ARGCHK(c && logits && out, "null argument"); ARGCHK(M > 0 && V > 0, "bad shape %d x %d", M, V);
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    for (int r = 0; ids && r < M; r++) ARGCHK(ids[r] >= 0 && ids[r] < V, "row %d: id %d outside the %d columns", r, ids[r], V);
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream; DevBuf dx, di, dout;
    HIPCHK(dout.alloc_pooled(c, (size_t)M * sizeof(TokenScore)));
    if (mem_kind == VOX_MEM_HOST) {
        HIPCHK(dx.alloc_pooled(c, (size_t)M * V * 4)); HIPCHK(hipMemcpyAsync(dx.p, logits, (size_t)M * V * 4, hipMemcpyHostToDevice, s)); logits = dx.as<float>();
    }
    if (ids) { HIPCHK(di.alloc_pooled(c, (size_t)M * 4)); HIPCHK(hipMemcpyAsync(di.p, ids, (size_t)M * 4, hipMemcpyHostToDevice, s)); }
    HIPCHK(launch_score_rows(logits, M, V, ids ? di.as<int>() : nullptr, dout.as<TokenScore>(), s));
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)M * sizeof(TokenScore), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    if (c->pw_model) return pw_after_sync(c->pw_model);      // (a synchronising call of the piecewise surface, as vox_argmax_rows)
    return VOX_OK;
}

// vox_score_rows' companion: a vox_token_alts per row (launch_alts_rows: the kernel the live sessions' alternatives come from).  Every check before the context is
// bound; host logits are uploaded.  out host; synchronises.
static_assert(sizeof(vox_token_alts) == 72 && sizeof(TokenAlts) == sizeof(vox_token_alts) && VOX_ALTS_MAX == VOX_MAX_ALTERNATIVES, "vox_token_alts is TokenAlts");
extern "C" int32_t vox_alternatives_rows(vox_ctx* c, const float* logits, int32_t M, int32_t V, int32_t k, vox_token_alts* out, int32_t mem_kind) {
    ARGCHK(c && logits && out, "null argument"); ARGCHK(M > 0 && V > 0, "bad shape %d x %d", M, V);
    ARGCHK(k >= 1 && k <= VOX_MAX_ALTERNATIVES, "k %d out of range (1..%d)", k, VOX_MAX_ALTERNATIVES);
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream; DevBuf dx, dout;
    HIPCHK(dout.alloc_pooled(c, (size_t)M * sizeof(TokenAlts)));
    if (mem_kind == VOX_MEM_HOST) {
        HIPCHK(dx.alloc_pooled(c, (size_t)M * V * 4)); HIPCHK(hipMemcpyAsync(dx.p, logits, (size_t)M * V * 4, hipMemcpyHostToDevice, s)); logits = dx.as<float>();
    }
    HIPCHK(launch_alts_rows(logits, M, V, k, dout.as<TokenAlts>(), s));
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)M * sizeof(TokenAlts), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    if (c->pw_model) return pw_after_sync(c->pw_model);      // (a synchronising call of the piecewise surface, as vox_score_rows)
    return VOX_OK;
}

// both records from one launch (launch_records_rows: the kernel the scored offline and batch calls take theirs from).  Every check before the context is bound; host
// logits are uploaded.  Records host; synchronises.
extern "C" int32_t vox_records_rows(vox_ctx* c, const float* logits, int32_t M, int32_t V, int32_t k, vox_token_score* scores, vox_token_alts* alts, int32_t mem_kind) {
    ARGCHK(c, "null context"); ARGCHK(logits, "null logits"); ARGCHK(M > 0 && V > 0, "bad shape %d x %d", M, V);
    VOXCHK(records_args_check(scores, alts, k));
    ARGCHK(k > 0 || scores, "k == 0 needs the scores array");
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream; DevBuf dx, dsc, dal;
    if (scores) HIPCHK(dsc.alloc_pooled(c, (size_t)M * sizeof(TokenScore)));
    if (alts) HIPCHK(dal.alloc_pooled(c, (size_t)M * sizeof(TokenAlts)));
    if (mem_kind == VOX_MEM_HOST) {
        HIPCHK(dx.alloc_pooled(c, (size_t)M * V * 4)); HIPCHK(hipMemcpyAsync(dx.p, logits, (size_t)M * V * 4, hipMemcpyHostToDevice, s)); logits = dx.as<float>();
    }
    HIPCHK(launch_records_rows(logits, M, V, k, dsc.as<TokenScore>(), dal.as<TokenAlts>(), s));
    if (scores) HIPCHK(hipMemcpyAsync(scores, dsc.p, (size_t)M * sizeof(TokenScore), hipMemcpyDeviceToHost, s));
    if (alts) HIPCHK(hipMemcpyAsync(alts, dal.p, (size_t)M * sizeof(TokenAlts), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (c->pw_model) return pw_after_sync(c->pw_model);      // (a synchronising call of the piecewise surface, as vox_score_rows)
    return VOX_OK;
}

// lm_head + argmax in one call: the token id comes back, not 512 KB of logits per row.  ids host; synchronises.
extern "C" int32_t vox_lm_head_argmax(vox_model* m, const float* hidden, int32_t M, int32_t* ids, int32_t mem_kind) {
    ARGCHK(m && hidden && ids && M > 0, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    if (m->pw_ids_cap < M) { if (m->pw_ids) HIPCHK(hipFree(m->pw_ids)); m->pw_ids = nullptr; m->pw_ids_cap = 0; const int cap = std::max(M, 64); HIPCHK(hipMalloc((void**)&m->pw_ids, (size_t)cap * 4)); m->pw_ids_cap = cap; }
    if (pw_memo_hit(m, hidden, M, mem_kind)) {
        HIPCHK(launch_argmax_final(m->eng_pw.part_val, m->eng_pw.part_idx, 256, m->pw_ids, nullptr, 0, 0, s));
    } else {
        const float* hx = hidden;
        if (mem_kind != VOX_MEM_DEVICE) { VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)M * c.dec_dim)); HIPCHK(hipMemcpyAsync(m->pw_x, hidden, (size_t)M * c.dec_dim * 4, hipMemcpyHostToDevice, s)); hx = m->pw_x; }
        VOXCHK(ensure(&m->pw_logits, &m->pw_logits_cap, (size_t)M * c.vocab)); m->pw_memo = false;
        VOXCHK(q4_linear_dev(m->ctx, m->tok.w, nullptr, hx, c.dec_dim, M, m->pw_logits, c.vocab));
        HIPCHK(launch_argmax_rows(m->pw_logits, M, c.vocab, m->pw_ids, s));
    }
    HIPCHK(hipMemcpyAsync(ids, m->pw_ids, (size_t)M * 4, hipMemcpyDeviceToHost, s));
    return pw_sync(m);
}

// Q4VoxtralModel::generate_step_with_cache (gguf/model.rs:857-867): decoder.forward_with_cache(token_ids) = embed + layers against the cache + final norm, then lm_head --
// one call, everything stays on the device between the three stages
extern "C" int32_t vox_generate_step_with_cache(vox_model* m, const int32_t* token_ids, int32_t n, const float* t_embed, vox_cache* kc, float* logits) {
    ARGCHK(m && token_ids && t_embed && kc && logits && n > 0, "bad argument"); ARGCHK(kc->m == m && kc->kind == 0, "cache belongs to another model or is an encoder cache"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    ARGCHK(kc->len + n <= kc->max_seq, "KV cache overflow: %d + %d > %d", kc->len, n, kc->max_seq);
    const int len0 = kc->len;
    VOXCHK(pw_ids_dev(m, token_ids, n));
    VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)n * c.dec_dim));
    HIPCHK(launch_embed(m->tok.w, m->pw_ids, n, nullptr, c.dec_dim, nullptr, 0, 0, m->pw_x, s));
    const float* hid = nullptr;
    VOXCHK(vox_forward_hidden_with_cache_ex(m, m->pw_x, n, t_embed, kc, nullptr, &hid, VOX_MEM_DEVICE));      // n == 1 on an eligible cache: one engine launch, logits included
    if (!pw_memo_hit(m, hid, n, VOX_MEM_DEVICE)) {
        VOXCHK(ensure(&m->pw_logits, &m->pw_logits_cap, (size_t)n * c.vocab));
        VOXCHK(q4_linear_dev(m->ctx, m->tok.w, nullptr, hid, c.dec_dim, n, m->pw_logits, c.vocab));
    }
    HIPCHK(hipMemcpyAsync(logits, m->pw_logits, (size_t)n * c.vocab * 4, hipMemcpyDeviceToHost, s));
    const int32_t r = pw_sync(m);
    if (r != VOX_OK) kc->len = std::min(kc->len, len0);
    return r;
}

// ---- composite forwards of Q4VoxtralModel (gguf/model.rs:802-843): mel -> logits in one call, composed of the pieces above -- nothing leaves the device in between.
// mode 0: forward (audio embeddings alone are the decoder input, :820-830); 1: forward_streaming (audio + embed(token_ids), :802-816); 2: forward_with_cache
// (encode_audio_with_cache + forward_hidden_with_cache against the caller's caches, :833-843).  logits [S][vocab]; *S = decoder positions.
static int32_t forward_composite(vox_model* m, int mode, const float* mel, int32_t T, const int32_t* token_ids, int32_t n_ids, const float* t_embed, vox_cache* enc_cache,
                                 vox_cache* dec_cache, float* logits, int32_t cap_rows, int32_t* S_out, int32_t mem_kind) {
    ARGCHK(m && mel && t_embed && logits && S_out && T > 0, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream; const int D = c.dec_dim;
    const float* d_mel = mel;
    if (mem_kind == VOX_MEM_HOST) {
        VOXCHK(ensure(&m->d_mel, &m->mel_cap, (size_t)c.n_mels * T));
        HIPCHK(hipMemcpyAsync(m->d_mel, mel, (size_t)c.n_mels * T * 4, hipMemcpyHostToDevice, s)); d_mel = m->d_mel;
    }
    int S = 0;
    if (mode == 2) {
        ARGCHK(enc_cache && dec_cache && enc_cache->kind == 1 && enc_cache->m == m && dec_cache->kind == 0 && dec_cache->m == m, "forward_with_cache needs an encoder and a decoder cache of this model");
        ARGCHK(cap_rows >= enc_rows(T) / c.reshape_factor, "logits capacity %d rows < %d", cap_rows, enc_rows(T) / c.reshape_factor);      // before anything is appended to the caches
        ARGCHK(dec_cache->len + enc_rows(T) / c.reshape_factor <= dec_cache->max_seq, "decoder cache overflow");
        VOXCHK(encode_with_cache_dev(m, d_mel, T, enc_cache, &S));
    } else {
        ARGCHK(cap_rows >= enc_rows(T) / c.reshape_factor, "logits capacity %d rows < %d", cap_rows, enc_rows(T) / c.reshape_factor);
        VOXCHK(encode_dev(m, d_mel, T, &S));
    }
    *S_out = S;
    if (S <= 0) { HIPCHK(hipStreamSynchronize(s)); return VOX_OK; }
    const float* x = m->d_audio;      // [S][D]
    if (mode == 1) {
        ARGCHK(token_ids && n_ids == S, "forward_streaming: %d token ids for %d audio positions", n_ids, S);
        VOXCHK(pw_ids_dev(m, token_ids, S));
        // audio_embeds + text_embeds (:810-812): the embedding kernel adds the audio rows itself
        VOXCHK(ensure(&m->pw_x, &m->pw_x_cap, (size_t)S * D));
        HIPCHK(launch_embed(m->tok.w, m->pw_ids, S, m->d_audio, D, nullptr, 0, 0, m->pw_x, s));
        x = m->pw_x;
    }
    vox_cache* kc = dec_cache; vox_cache* tmp = nullptr;
    if (mode != 2) { VOXCHK(cache_alloc(m, std::max(S, 8), &tmp)); kc = tmp; }      // forward_hidden(.., offset 0): a cache of exactly this call's rows
    auto decode_rows = [&]() -> int32_t {      // layers against the cache -> final norm -> lm_head -> logits on their way to the caller
        const float* hid = nullptr;
        int32_t r = vox_forward_hidden_with_cache_ex(m, x, S, t_embed, kc, nullptr, &hid, VOX_MEM_DEVICE);
        if (r != VOX_OK) return r;
        float* ly = logits;
        if (mem_kind == VOX_MEM_HOST) { r = ensure(&m->pw_logits, &m->pw_logits_cap, (size_t)S * c.vocab); ly = m->pw_logits; m->pw_memo = false; }
        if (r == VOX_OK && !(pw_memo_hit(m, hid, S, VOX_MEM_DEVICE) && ly == m->pw_logits)) {
            if (pw_memo_hit(m, hid, S, VOX_MEM_DEVICE)) { if (hipMemcpyAsync(ly, m->pw_logits, (size_t)c.vocab * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) r = fail(VOX_ERR_HIP, "copy of the logits failed"); }
            else r = q4_linear_dev(m->ctx, m->tok.w, nullptr, hid, D, S, ly, c.vocab);
        }
        if (r == VOX_OK && mem_kind == VOX_MEM_HOST && hipMemcpyAsync(logits, ly, (size_t)S * c.vocab * 4, hipMemcpyDeviceToHost, s) != hipSuccess) r = fail(VOX_ERR_HIP, "copy of the logits failed");
        return r;
    };
    // settle whatever earlier piecewise steps left unverified BEFORE this call's rows: a failed verdict found behind decode_rows() must be about THIS call's rows for the
    // silent re-run below to be right -- an earlier step's failure belongs to its owner (whose cache was just shortened) and is reported
    if (m->pw_pend_rows > 0) { const int32_t r0 = pw_sync(m); if (r0 != VOX_OK) { if (tmp) (void)vox_cache_free(tmp); return r0; } }
    m->pw_verdict_failed = false;
    int32_t r = decode_rows();
    int32_t rs = pw_sync(m);
    if (m->pw_verdict_failed) {
        // an engine hand-off timeout (a one-row call on a shared GPU): the verdict has taken the decoder row back; the ENCODER cache of mode 2 cannot be rewound (it may have
        // compacted itself), so the call is not failed -- the decoder rows run once more on the per-operator launches and the caller never sees a half-advanced pair of caches
        m->pw_verdict_failed = false;
        EngSuspend off(m);
        r = decode_rows(); rs = pw_sync(m);
    }
    if (tmp) (void)vox_cache_free(tmp);
    return r != VOX_OK ? r : rs;
}
extern "C" int32_t vox_forward(vox_model* m, const float* mel, int32_t T, const float* t_embed, float* logits, int32_t cap_rows, int32_t* S, int32_t mem_kind) {
    return forward_composite(m, 0, mel, T, nullptr, 0, t_embed, nullptr, nullptr, logits, cap_rows, S, mem_kind);
}
extern "C" int32_t vox_forward_streaming(vox_model* m, const float* mel, int32_t T, const int32_t* token_ids, int32_t n_ids, const float* t_embed, float* logits, int32_t cap_rows,
                                         int32_t* S, int32_t mem_kind) {
    return forward_composite(m, 1, mel, T, token_ids, n_ids, t_embed, nullptr, nullptr, logits, cap_rows, S, mem_kind);
}
extern "C" int32_t vox_forward_with_cache(vox_model* m, const float* mel, int32_t T, const float* t_embed, vox_cache* enc_cache, vox_cache* dec_cache, float* logits, int32_t cap_rows,
                                          int32_t* S, int32_t mem_kind) {
    return forward_composite(m, 2, mel, T, nullptr, 0, t_embed, enc_cache, dec_cache, logits, cap_rows, S, mem_kind);
}

extern "C" int32_t vox_get_stage_timings(const vox_model* m, vox_timings* out) { ARGCHK(m && out, "null argument"); *out = m->timings; return VOX_OK; }

// ---- measurement hook: average launch duration of one decode-step GEMV class, HIP events on the ctx stream
// measurement hook of the wide decode step (tools/wide_bench.py): operator `which` (0 q|k|v, 1 wo, 2 w1|w3, 3 w2, 4 lm_head) for `mt` slot groups, `iters` launches cycling the
// layers (weights HBM-cold); out_us[0] the GEMM launch alone, [1] the finishing launch alone, [2] both back to back, [3] the same operator as `mt` launches of the 16-row
// skinny kernel back to back on one stream (what a forked chain issues per group)
extern "C" int32_t vox_bench_wide(vox_model* m, int32_t which, int32_t mt, int32_t iters, double out_us[4]) {
    ARGCHK(m && out_us && iters > 0 && which >= 0 && which <= 4 && mt >= 2 && mt <= 4, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const int D = c.dec_dim, H = c.dec_heads, KV = c.dec_kv_heads, hd = c.dec_head_dim, QD = H * hd, KD = KV * hd, W = QD + 2 * KD, F = c.dec_ffn, V = c.vocab, Sl = 16 * mt, max_seq = 256;
    ARGCHK(batch_xf_ok(m), "the model has no tile-ordered Q4 weights");
    if (!m->t_embed_set) { std::vector<float> te(D); vox_time_embedding(6.0f, D, te.data()); VOXCHK(vox_model_set_t_embed(m, te.data())); }
    auto xf_bytes = [](int K) { return (size_t)2 * (K / 128) * 256 * 16; };
    const int parts_D = q4_skinny_resid_xf_parts(D);
    const size_t seq_stride = (size_t)KV * max_seq * hd;
    DevBuf b_xf, b_xfo, b_ssq, b_h, b_qkv, b_k, b_v, b_pos, b_row, b_planes, b_logits;
    size_t planes_bytes = 0;
    const Q4W* w0[5] = {&m->dec[0].wqkv.w, &m->dec[0].wo.w, &m->dec[0].w13.w, &m->dec[0].w2.w, &m->tok.w};
    const int epis[5] = {EPI_ROPE_KV, EPI_RESID_XF, EPI_SWIGLU_XF, EPI_RESID_XF, EPI_STORE};
    WidePlan pl; ARGCHK(q4_wide_plan(*w0[which], mt, epis[which], &pl), "no wide plan for this shape");
    planes_bytes = q4_wide_planes_bytes(*w0[which], mt, pl);
    HIPCHK(b_xf.alloc(xf_bytes(F) * 4)); HIPCHK(b_xfo.alloc(xf_bytes(F) * 4)); HIPCHK(b_ssq.alloc((size_t)parts_D * 16 * 4 * 4)); HIPCHK(b_h.alloc((size_t)Sl * D * 4)); HIPCHK(b_qkv.alloc((size_t)Sl * W * 4));
    HIPCHK(b_k.alloc((size_t)Sl * seq_stride * 4)); HIPCHK(b_v.alloc((size_t)Sl * seq_stride * 4)); HIPCHK(b_pos.alloc((size_t)Sl * 4)); HIPCHK(b_row.alloc((size_t)Sl * 4)); HIPCHK(b_planes.alloc(std::max<size_t>(planes_bytes, 16)));
    if (which == 4) HIPCHK(b_logits.alloc((size_t)Sl * V * 4));
    {   // random bf16 activations (hi planes ~ N(0,1)-ish magnitudes, lo planes small): all-zero operands run at a higher clock (DVFS), which would flatter the kernel
        std::vector<uint16_t> hx(xf_bytes(F) * 4 / 2); uint32_t r = 12345u;
        for (auto& v : hx) { r = r * 1664525u + 1013904223u; v = (uint16_t)(((r >> 16) & 0x8000u) | 0x3F00u | ((r >> 8) & 0xFFu)); }      // +-[0.5, 2)
        HIPCHK(hipMemcpy(b_xf.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
        std::vector<float> one((size_t)parts_D * 16 * 4, 3.0f); HIPCHK(hipMemcpy(b_ssq.p, one.data(), one.size() * 4, hipMemcpyHostToDevice));
        std::vector<int> pos(Sl, 100), row(Sl); for (int i = 0; i < Sl; i++) row[i] = i;
        HIPCHK(hipMemcpy(b_pos.p, pos.data(), (size_t)Sl * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(b_row.p, row.data(), (size_t)Sl * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(b_h.p, 0, (size_t)Sl * D * 4));
    }
    auto params = [&](int l, bool wide, int gi) {
        const DecLayer& L = m->dec[l % c.dec_layers];
        const Q4W& w = which == 0 ? L.wqkv.w : which == 1 ? L.wo.w : which == 2 ? L.w13.w : which == 3 ? L.w2.w : m->tok.w;
        const int K = w.K;
        GemmParams g{}; g.w = w; g.norm_eps = c.norm_eps;
        const size_t go = wide ? 0 : (size_t)gi;      // skinny launches: group gi's planes / rows
        g.xf = (const uint4*)((const uint8_t*)b_xf.p + go * xf_bytes(K)); g.M = wide ? Sl : 16;
        if (wide) { g.xf_gstride = (long)(xf_bytes(K) / 16); g.wide_mt = mt; g.kz_scratch = b_planes.as<float>(); g.kz_scratch_bytes = planes_bytes; }
        float* ssq = b_ssq.as<float>() + go * parts_D * 16; float* hg = b_h.as<float>() + go * 16 * D;
        switch (which) {
        case 0: g.out = b_qkv.as<float>() + go * 16 * W; g.out_stride = W; g.ssq_part = ssq; g.ssq_part_gstride = (long)parts_D * 16; g.n_part = parts_D; g.pos = b_pos.as<int>() + go * 16; g.kv_row = b_row.as<int>() + go * 16;
                g.rope_cos = m->dec_cos; g.rope_sin = m->dec_sin; g.hd = hd; g.n_q = QD; g.n_kv = KV; g.kc = b_k.as<float>(); g.vc = b_v.as<float>(); g.kv_seq_stride = (long)seq_stride; g.kv_head_stride = max_seq * hd; break;
        case 1: case 3: g.out = hg; g.out_stride = D; g.resid = hg; g.resid_stride = D; g.xf_out = (uint16_t*)((uint8_t*)b_xfo.p + go * xf_bytes(D)); g.xf_out_gstride = (long)(xf_bytes(D) / 2); g.xf_w = L.ffn_norm; g.xf_w2 = which == 1 ? L.ada_mul : nullptr;
                g.ssq_out = ssq; g.ssq_out_gstride = (long)parts_D * 16; break;
        case 2: g.out = (float*)((uint8_t*)b_xfo.p + go * xf_bytes(F)); g.out_stride = F; g.xf_out_gstride = (long)(xf_bytes(F) / 2); g.ssq_part = ssq; g.ssq_part_gstride = (long)parts_D * 16; g.n_part = parts_D; break;
        default: g.out = b_logits.as<float>() + go * 16 * V; g.out_stride = V; g.ssq_part = ssq; g.ssq_part_gstride = (long)parts_D * 16; g.n_part = parts_D; break;
        }
        return g;
    };
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    auto timed = [&](int mode, double* us) -> int32_t {
        for (int rep = 0; rep < 2; rep++) {      // (first repetition: warm-up)
            HIPCHK(hipEventRecord(e0, s));
            for (int i = 0; i < iters; i++) {
                if (mode < 3) { const GemmParams g = params(i, true, 0); HIPCHK(launch_q4_wide(g, epis[which] | (mode == 0 ? 0x100 : mode == 1 ? 0x200 : 0), s)); }
                else for (int gi = 0; gi < mt; gi++) { const GemmParams g = params(i, false, gi); HIPCHK(launch_q4_gemm(g, epis[which], s)); }
            }
            HIPCHK(hipEventRecord(e1, s)); HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1)); *us = (double)ms * 1000.0 / iters;
        }
        return VOX_OK;
    };
    out_us[1] = 0.0;
    VOXCHK(timed(0, &out_us[0])); if (which != 4) VOXCHK(timed(1, &out_us[1])); VOXCHK(timed(2, &out_us[2])); VOXCHK(timed(3, &out_us[3]));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}

extern "C" int32_t vox_bench_decode_gemv(vox_model* m, int32_t which, int32_t iters, double* avg_us, double* bytes_per_launch, const char** kernel_name) {
    const bool warm = (which & 0x100) != 0;   // measurement variant: same layer every launch (weights stay in L2 / Infinity Cache)
    which &= 0xff;
    ARGCHK(m && avg_us && bytes_per_launch && iters > 0 && which >= 0 && which <= 5, "bad argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream;
    VOXCHK(ensure_decode_state(m, 64));
    if (which == 5) {      // the whole decode step as ONE launch of the persistent engine, at the positions the 16 s bench clip decodes at (38 .. 145: four equal shares at 40, 75,
        // 110, 145 -- the step gets longer with the position, a single low position would overstate the in-product rate)
        if (!m->t_embed_set) { std::vector<float> te(c.dec_dim); vox_time_embedding(6.0f, c.dec_dim, te.data()); VOXCHK(vox_model_set_t_embed(m, te.data())); }
        if (!engine_bind(m, m->eng_offline, m->cache)) return fail(VOX_ERR_UNSUPPORTED, "decode engine not active for this model / device");
        static const int bench_pos[4] = {40, 75, 110, 145};
        HIPCHK(hipMemcpyAsync(m->d_pos, &bench_pos[0], 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(m->d_h, 0, (size_t)c.dec_dim * 4, s));
        double bytes = 0; for (const Q4W* w : {&m->dec[0].wqkv.w, &m->dec[0].wo.w, &m->dec[0].w13.w, &m->dec[0].w2.w}) bytes += (double)w->N * w->nb * 18.0;
        *bytes_per_launch = bytes * c.dec_layers + (double)m->tok.w.N * m->tok.w.nb * 18.0;
        if (kernel_name) *kernel_name = "decode_engine_kernel";
        const int per_q = std::max(iters / 4, 1);
        VOXCHK(engine_take_serials(m, 4ull * per_q + 3, s));      // three warm-up launches + four timed quarters
        const EngParams ep = engine_params(m, m->eng_offline, m->cache, m->d_h, m->d_pos, 0, nullptr);
        for (int i = 0; i < 3; i++) HIPCHK(launch_decode_engine(ep, s));
        // one event pair per quarter, around the LAUNCHES only: the position update between the quarters (a 4-byte copy from pageable host memory: 20 - 250 us depending on
        // the box) used to sit inside the timed region -- 603 us per launch on one box, 628 on another where rocprofv3 saw 605 (round 6)
        // ... and the launches of a quarter go out as ONE graph replay, the way the product issues its steps (on some boxes ten plain launches in a row cost 25 us more per
        // launch than the same ten in a graph: 629 against 603 us where the product's own steps took 596)
        hipEvent_t ev[8]; for (auto& e : ev) HIPCHK(hipEventCreate(&e));
        hipGraph_t gq = nullptr; hipGraphExec_t gx = nullptr;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        hipError_t ce = hipSuccess; for (int i = 0; i < per_q && ce == hipSuccess; i++) ce = launch_decode_engine(ep, s);
        const hipError_t ee = hipStreamEndCapture(s, &gq);
        if (ce != hipSuccess || ee != hipSuccess || hipGraphInstantiate(&gx, gq, nullptr, nullptr, 0) != hipSuccess) { if (gq) (void)hipGraphDestroy(gq); for (auto& e : ev) (void)hipEventDestroy(e); return fail(VOX_ERR_HIP, "engine timing: graph capture failed"); }
        for (int q = 0; q < 4; q++) {
            const int pq = std::min(bench_pos[q], m->cache->max_seq - 2);
            HIPCHK(hipMemcpyAsync(m->d_pos, &pq, 4, hipMemcpyHostToDevice, s));      // (pageable host source: staged at call time)
            HIPCHK(hipEventRecord(ev[2 * q], s));
            HIPCHK(hipGraphLaunch(gx, s));
            HIPCHK(hipEventRecord(ev[2 * q + 1], s));
        }
        HIPCHK(hipEventSynchronize(ev[7]));
        float ms = 0.f; for (int q = 0; q < 4; q++) { float mq = 0.f; HIPCHK(hipEventElapsedTime(&mq, ev[2 * q], ev[2 * q + 1])); ms += mq; }
        for (auto& e : ev) (void)hipEventDestroy(e);
        (void)hipGraphExecDestroy(gx); (void)hipGraphDestroy(gq);
        iters = 4 * per_q;
        *avg_us = (double)ms * 1000.0 / iters;
        unsigned err2[2] = {0, 0}; HIPCHK(hipMemcpy(err2, ep.err, 8, hipMemcpyDeviceToHost));
        if (err2[0]) return fail(VOX_ERR_HIP, "decode engine: %s", engine_timeout_text(err2[0], 0).c_str());
        return VOX_OK;
    }
    const int zero = 0; HIPCHK(hipMemcpyAsync(m->d_pos, &zero, 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(m->d_h, 0, (size_t)c.dec_dim * 4, s)); HIPCHK(hipMemsetAsync(m->d_att, 0, (size_t)c.dec_heads * c.dec_head_dim * 4, s));
    HIPCHK(hipMemsetAsync(m->d_act, 0, (size_t)c.dec_ffn * 4, s));
    if (!m->t_embed_set) { std::vector<float> te(c.dec_dim); vox_time_embedding(6.0f, c.dec_dim, te.data()); VOXCHK(vox_model_set_t_embed(m, te.data())); }
    const int D = c.dec_dim, QD = c.dec_heads * c.dec_head_dim, KD = c.dec_kv_heads * c.dec_head_dim, F = c.dec_ffn, hd = c.dec_head_dim;
    const size_t lf = m->cache->layer_stride;
    bool fused = false;
    { AttnParams ap{}; ap.n_heads = c.dec_heads; ap.n_kv_heads = c.dec_kv_heads; ap.kv_row_stride = hd; ap.kv_head_stride = m->cache->max_seq * hd;
      fused = decode_layer_fuses_attn_wo(m, m->dec[0], ap, m->cache); if (fused) VOXCHK(wo_acc_clear(m, s)); }
    auto launch = [&](int l) -> int32_t {
        if (warm) l = 0;
        const DecLayer& L = m->dec[l % c.dec_layers]; GemvParams p{};
        switch (which) {
        case 0: p.w = L.wqkv.w; p.x = m->d_h; p.x_stride = D; p.out = m->d_q; p.out_stride = QD; p.gamma = L.attn_norm; p.eps = c.norm_eps; p.pos_ptr = m->d_pos;
                p.rope_cos = m->dec_cos; p.rope_sin = m->dec_sin; p.hd = hd; p.n_q = QD; p.n_k = KD; p.kcache = m->cache->k + (size_t)(l % c.dec_layers) * lf;
                p.vcache = m->cache->v + (size_t)(l % c.dec_layers) * lf; p.cache_head_stride = m->cache->max_seq * hd;
                HIPCHK(launch_q4_gemv(p, 1, PRO_RMS, EPI_ROPE_KV, q4_gemv_default_R(p.w.N, p.w.K, EPI_ROPE_KV), s)); break;
        case 1: p.w = L.wo.w; p.x = m->d_att; p.x_stride = QD; p.out = m->d_h; p.out_stride = D; p.resid = m->d_h; p.resid_stride = D;
                HIPCHK(launch_q4_gemv(p, 1, PRO_NONE, EPI_RESID, q4_gemv_default_R(p.w.N, p.w.K, EPI_RESID), s)); break;
        case 2: p.w = L.w13.w; p.x = m->d_h; p.x_stride = D; p.out = m->d_act; p.out_stride = F; p.gamma = L.ffn_norm; p.mul = L.ada_mul; p.eps = c.norm_eps;
                if (fused) { p.xacc = m->d_wo_acc + (size_t)(l % c.dec_layers) * D; p.x_out = m->d_h2; }      // as launched by the decode step (accumulators: zeros)
                HIPCHK(launch_q4_gemv(p, 1, fused ? PRO_RMS_MUL_SUM : PRO_RMS_MUL, EPI_SWIGLU, q4_gemv_default_R(p.w.N, p.w.K, EPI_SWIGLU), s)); break;
        case 3: p.w = L.w2.w; p.x = m->d_act; p.x_stride = F; p.out = m->d_h; p.out_stride = D; p.resid = m->d_h; p.resid_stride = D;
                HIPCHK(launch_q4_gemv(p, 1, PRO_NONE, EPI_RESID, q4_gemv_default_R(p.w.N, p.w.K, EPI_RESID), s)); break;
        default: VOXCHK(lm_head_argmax_dev(m, m->d_h, nullptr)); break;
        }
        return VOX_OK;
    };
    const Q4W* w = which == 0 ? &m->dec[0].wqkv.w : which == 1 ? &m->dec[0].wo.w : which == 2 ? &m->dec[0].w13.w : which == 3 ? &m->dec[0].w2.w : &m->tok.w;
    *bytes_per_launch = w->fmt == WFMT_BF16 ? (double)w->N * w->K * 2.0 : w->fmt == WFMT_F32 ? (double)w->N * w->K * 4.0 : (double)w->N * w->nb * 18.0;   // algorithmic bytes: Q4_0 blocks (18 B / 32 weights) or bf16
    if (kernel_name) {
        const int epi = which == 0 ? EPI_ROPE_KV : which == 2 ? EPI_SWIGLU : which == 4 ? EPI_ARGMAX : EPI_RESID;
        const int pro = which == 2 ? (fused ? PRO_RMS_MUL_SUM : PRO_RMS_MUL) : (which == 0 || which == 4) ? PRO_RMS : PRO_NONE;
        if (w->fmt == WFMT_BF16 || w->fmt == WFMT_F32) { static thread_local char nb_[64]; snprintf(nb_, sizeof nb_, "dense_gemv_kernel<PRO=%d,EPI=%d>", pro, epi); *kernel_name = nb_; }
        else *kernel_name = q4_gemv_kernel_name(w->K, pro, epi, which == 4 ? m->argmax_R : q4_gemv_default_R(w->N, w->K, epi));
    }
    for (int i = 0; i < std::min(iters, 8); i++) VOXCHK(launch(i));   // warm-up
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; i++) VOXCHK(launch(i));
    HIPCHK(hipEventRecord(e1, s)); HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = (double)ms * 1000.0 / iters;
    return VOX_OK;
}

// ---- measurement hook (timeline builds, -DVOX_TIMELINE): per-wave s_memrealtime stamps of every decode-step GEMV / attention launch
static unsigned long long* g_tl_dev = nullptr; static int g_tl_nslots = 0, g_tl_nwaves = 0;
extern "C" int32_t vox_debug_timeline_start(vox_ctx* c, int32_t n_slots, int32_t n_waves) {
    ARGCHK(c && n_slots > 0 && n_waves > 0, "bad argument"); VOXCHK(ctx_bind(c));
    if (g_tl_dev) { (void)tl_configure(nullptr, 0, 0); (void)hipFree(g_tl_dev); g_tl_dev = nullptr; }
    const size_t bytes = (size_t)n_slots * n_waves * 4 * sizeof(unsigned long long);
    HIPCHK(hipMalloc((void**)&g_tl_dev, bytes)); HIPCHK(hipMemset(g_tl_dev, 0, bytes));
    if (tl_configure(g_tl_dev, n_slots, n_waves) != hipSuccess) { (void)hipFree(g_tl_dev); g_tl_dev = nullptr; return fail(VOX_ERR_UNSUPPORTED, "library built without -DVOX_TIMELINE"); }
    g_tl_nslots = n_slots; g_tl_nwaves = n_waves; return VOX_OK;
}
extern "C" int32_t vox_debug_timeline_fetch(vox_ctx* c, uint64_t* out, size_t cap_words, int32_t* slots_used, int32_t* meta) {
    ARGCHK(c && out && slots_used, "null argument"); VOXCHK(ctx_bind(c));
    if (meta) for (int i = 0; i < g_tl_nslots; i++) tl_slot_meta(i, meta + 4 * i);
    ARGCHK(g_tl_dev, "timeline not started");
    const size_t words = (size_t)g_tl_nslots * g_tl_nwaves * 4;
    ARGCHK(cap_words >= words, "timeline output buffer too small (%zu < %zu words)", cap_words, words);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, g_tl_dev, words * 8, hipMemcpyDeviceToHost));
    *slots_used = tl_slots_used();
    (void)tl_configure(nullptr, 0, 0); (void)hipFree(g_tl_dev); g_tl_dev = nullptr;
    return VOX_OK;
}

// ---- debug: per-unit logits tap of the batched decoder (BatchTapCall, launch_batch_tap)
static void tap_release(vox_model* m) {
    if (m->tap.out || m->tap.rows) (void)hipSetDevice(m->ctx->device);
    if (m->tap.out) (void)hipFree(m->tap.out);
    if (m->tap.rows) (void)hipFree(m->tap.rows);
    m->tap.out = nullptr; m->tap.rows = nullptr; m->tap.armed = m->tap.ready = false;
}
extern "C" int32_t vox_debug_batch_tap_arm(vox_model* m, const int32_t* units, int32_t n_units, int32_t max_rows) {
    ARGCHK(units && n_units > 0 && n_units <= 4096, "bad tap unit list (%d units)", n_units); ARGCHK(max_rows > 0 && max_rows <= 65536, "max_rows %d out of range (1..65536)", max_rows);
    ARGCHK(m, "null model");
    std::vector<int> u(units, units + n_units);
    for (int i = 0; i < n_units; i++) { ARGCHK(u[i] >= 0, "tapped unit %d < 0", u[i]); for (int j = 0; j < i; j++) ARGCHK(u[j] != u[i], "unit %d tapped twice", u[i]); }
    tap_release(m);
    m->tap.units = u; m->tap.max_rows = max_rows; m->tap.armed = true;
    return VOX_OK;
}
extern "C" int32_t vox_debug_batch_tap_fetch(vox_model* m, float* out, int32_t* rows_per_unit) {
    ARGCHK(m && out && rows_per_unit, "null argument");
    if (!m->tap.ready) { tap_release(m); return fail(VOX_ERR_INVALID, "no batch tap to fetch (arm one, then make one successful vox_transcribe_batch call)"); }
    VOXCHK(ctx_bind(m->ctx));
    const size_t nu = m->tap.units.size();
    HIPCHK(hipDeviceSynchronize());
    const hipError_t e1 = hipMemcpy(out, m->tap.out, nu * (size_t)m->tap.max_rows * m->cfg.vocab * 4, hipMemcpyDeviceToHost);
    const hipError_t e2 = hipMemcpy(rows_per_unit, m->tap.rows, nu * 4, hipMemcpyDeviceToHost);
    tap_release(m);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(VOX_ERR_HIP, "batch tap copy failed");
    return VOX_OK;
}

// ---- debug: one encoder stack exactly as a batch driver runs it (encode_batch_dev), the adapter rows of every clip copied back with the forms the stack took
extern "C" int32_t vox_debug_encode_batch(vox_model* m, int32_t n, const float* const* mels, const int32_t* T, int32_t layout, float* out, int64_t cap_rows,
                                          int32_t* rows_per_clip, int64_t* report) {
    ARGCHK(m, "null model");
    ARGCHK(n > 0 && n <= 128, "encoder stack of %d clips out of range (1..128)", n);
    ARGCHK(layout == 0 || layout == 1, "layout %d: 0 padded, 1 packed", layout);
    ARGCHK(mels && T && out && rows_per_clip && report, "null argument");
    for (int i = 0; i < n; i++) ARGCHK(mels[i] && T[i] > 0, "clip %d: empty mel", i);
    const vox_model_cfg& c = m->cfg; const int R = c.reshape_factor, D = c.dec_dim, PREFIX_LEN = 38;
    const std::vector<int> Ti(T, T + n);
    long need_rows = 0; for (int i = 0; i < n; i++) need_rows += enc_rows(Ti[i]) / R;
    ARGCHK(cap_rows >= need_rows, "output capacity %lld rows < %ld", (long long)cap_rows, need_rows);
    VOXCHK(ctx_bind(m->ctx)); hipStream_t s = m->ctx->stream;
    size_t mel_floats = 0; for (int i = 0; i < n; i++) mel_floats += (size_t)c.n_mels * Ti[i];
    // the audio buffer as the drivers size it: padded = n budgets of audio_rows rows (transcribe_batch_impl), packed = every clip's packed rows / R back to back
    int audio_rows = 0; size_t audio_floats = 0; std::vector<long> off(n, 0);
    if (layout == 0) { audio_rows = std::max(enc_row_budget(m, Ti.data(), n) / R, PREFIX_LEN + 1); audio_floats = (size_t)n * audio_rows * D; for (int i = 0; i < n; i++) off[i] = (long)i * audio_rows * D; }
    else audio_floats = (size_t)(enc_packed_rows(m, Ti.data(), n) / R) * D;
    DevBuf b_mel, b_audio;
    HIPCHK(b_mel.alloc(mel_floats * 4)); HIPCHK(b_audio.alloc(audio_floats * 4));
    HIPCHK(hipMemsetAsync(b_audio.p, 0, audio_floats * 4, s));
    std::vector<const float*> d_mels(n); size_t mo = 0;
    for (int i = 0; i < n; i++) {
        float* d = b_mel.as<float>() + mo; mo += (size_t)c.n_mels * Ti[i];
        HIPCHK(hipMemcpyAsync(d, mels[i], (size_t)c.n_mels * Ti[i] * 4, hipMemcpyHostToDevice, s)); d_mels[i] = d;
    }
    std::vector<int> S4(n, 0); EncForms f;
    VOXCHK(encode_batch_dev(m, n, d_mels.data(), Ti.data(), b_audio.as<float>(), audio_rows, S4.data(), layout == 1 ? off.data() : nullptr, &f));
    HIPCHK(hipStreamSynchronize(s));
    size_t o = 0;
    for (int i = 0; i < n; i++) {
        if (S4[i] > 0) HIPCHK(hipMemcpy(out + o, b_audio.as<float>() + off[i], (size_t)S4[i] * D * 4, hipMemcpyDeviceToHost));
        o += (size_t)S4[i] * D; rows_per_clip[i] = S4[i];
    }
    report[0] = f.Mtot; report[1] = f.ksp; report[2] = f.ksp_wo; report[3] = f.fused_rope;
    return VOX_OK;
}

// ------------------------------------------------------------------------------------------------
// Live streaming session (vox_stream).  16 kHz samples go in in pieces of any size, token ids come back as soon as they are determined, and the
// concatenation of everything handed back is what vox_transcribe_streaming gives for the log-mel of pad_audio(gain * samples).
// The session always advances in TICKS of one decoder position -- 4 R mel frames -> R encoder rows -> 1 adapter row -> 1 decode step -- however the samples were cut
// into pushes: a large push is a loop of identical ticks, so the ids (and which call returns which) are a function of the samples and the gain alone.  It starts from
// the model's prefix state (encoder rows 0 .. RC-1, decoder positions 0 .. PC-1 of the silent left pad): a live session starts where the silence ends.
//   schedule: decoder position p is determined once its last mel frame 4 R p + 4 R - 1 is, i.e. once left + n >= 640 R (p + 1) + 40 padded samples exist;
//   per tick: stream_mel_kernel (4 R new frames + 3 halo frames, token-major) -> conv stem as two small im2col GEMMs on the halo buffer -> enc_layers x { RMSNorm,
//   q|k|v GEMV, stream_attn_kernel (RoPE + ring append + windowed attention), wo, RMSNorm, w1|w3, w2 } -> final norm, adapter -> stream_embed_kernel -> one decode step
//   (engine launch while the stream's decoder cache has <= 1024 rows, per-operator launches after) -> stream_advance_kernel (token, state block).
// Ingest at the capture rate (vox_stream_create_rate): input-rate samples go into a ring of their own, stream_resample_kernel turns every block that
// is complete into 16 kHz samples of the ring above (vox_resample's bits: the same matrix, the same sums), the ticks see 16 kHz samples only.  16-bit PCM
// (vox_stream_push_s16) is converted on the device on its way into whichever ring the stream is fed through.
// What a call appends, resamples, pads and ticks, pass by pass, is decided by feed_plan / feed_pass on the stream's FeedState -- the planner a group's members share.
// ONE call path: push, finish and peek are stream_run (a group's advance and peek: group_run), which hands the call's ids and score records back through SessionOut
// around the call's one synchronisation; a peek is the mode of it that runs between the two directions of the ring keep (ring_keep) and ends in FeedState::rewind.
// ------------------------------------------------------------------------------------------------
static const int STREAM_KEEP_ROWS = 1024;           // adapter rows kept for the re-run of unverified engine steps; a push verifies at least this often
// A session's scores (vox_stream_set_scores; DESIGN.md section 8, "Scores"): the device records the score kernel writes, one per id of the utterance, and their host
// mirror -- one record per id handed out, the ones of a call copied in front of its synchronisation.  Nothing is allocated before the first set(1).
// a position-indexed device list of `*cap` records of `rec` bytes grows to `rows` records: a new array, the old records copied on the stream, the old array freed behind
// a synchronisation (nothing may still read it)
static int32_t list_grow(void** dev, int* cap, int rows, size_t rec, hipStream_t s) {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)rows * rec) != hipSuccess) { (void)hipGetLastError(); return fail(VOX_ERR_HIP, "hipMalloc of a session's %d-record list failed", rows); }
    hipError_t e = hipMemcpyAsync(q, *dev, (size_t)*cap * rec, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(q); return fail(VOX_ERR_HIP, "growing a session's list failed: %s", hipGetErrorString(e)); }
    (void)hipFree(*dev); *dev = q; *cap = rows;
    return VOX_OK;
}
struct ScoreState {
    bool on = false; TokenScore* dev = nullptr; int cap = 0;
    std::vector<vox_token_score> host;
    size_t bytes() const { return dev ? (size_t)cap * sizeof(TokenScore) : 0; }
    // the first set(1): the device records of a session of max_pos positions.  `whose`: the message's subject ("the stream's", "member 3's")
    int32_t alloc(int max_pos, const char* whose) {
        if (dev) return VOX_OK;
        if (hipMalloc((void**)&dev, (size_t)(max_pos + 2) * sizeof(TokenScore)) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of %s score records failed", whose); }
        cap = max_pos + 2; return VOX_OK;
    }
    // an endless session's records outgrow their array: `rows` records from here on, the old ones copied over (the caller synchronises and points its descriptor at dev)
    int32_t grow(int rows, hipStream_t s) { return list_grow((void**)&dev, &cap, rows, sizeof(TokenScore), s); }
    // in front of the call's synchronisation: the copy of the call's `due` records behind the `have` handed out so far, when scores are on and there is a destination
    int32_t enqueue(int have, int due, vox_token_score* dst, hipStream_t s) const {
        if (on && dst && due > 0) HIPCHK(hipMemcpyAsync(dst, dev + have, (size_t)due * sizeof(TokenScore), hipMemcpyDeviceToHost, s));
        return VOX_OK;
    }
    // behind it: the ids of a call that ran with scores off get the records that say so
    void settle(int due, const int32_t* ids, vox_token_score* dst) const {
        const float nan = NAN;
        for (int i = 0; !on && dst && i < due; i++) dst[i] = vox_token_score{nan, nan, -1, ids[i]};
    }
    int32_t read(int have, int32_t first_id, int32_t n, vox_token_score* out) const {
        ARGCHK(first_id >= 0 && n >= 0 && (int64_t)first_id + n <= have, "%d ids from %d on: %d handed out", n, first_id, have);
        ARGCHK(out || n == 0, "null output");
        if (n > 0) std::memcpy(out, host.data() + first_id, (size_t)n * sizeof(vox_token_score));
        return VOX_OK;
    }
};
// A session's alternatives (vox_stream_set_alternatives; DESIGN.md section 8, "Alternatives"): ScoreState's twin for the 72-byte records, at the session's k (0: off).
// peeked: the records of the ids the last peek returned -- never part of the session's list, gone with the next push / finish / peek / reset.
struct AltsState {
    int k = 0; TokenAlts* dev = nullptr; int cap = 0;
    std::vector<vox_token_alts> host, peeked;
    size_t bytes() const { return dev ? (size_t)cap * sizeof(TokenAlts) : 0; }
    static vox_token_alts off() { vox_token_alts r; r.entropy = NAN; r.n = 0; for (vox_alt& a : r.alt) a = vox_alt{-1, NAN}; return r; }
    int32_t alloc(int max_pos, const char* whose) {      // the first k > 0
        if (dev) return VOX_OK;
        if (hipMalloc((void**)&dev, (size_t)(max_pos + 2) * sizeof(TokenAlts)) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of %s alternatives records failed", whose); }
        cap = max_pos + 2; return VOX_OK;
    }
    int32_t grow(int rows, hipStream_t s) { return list_grow((void**)&dev, &cap, rows, sizeof(TokenAlts), s); }      // as ScoreState::grow
    void restart() { host.clear(); peeked.clear(); }      // create / reset: the lists start over, k stays
    // in front of the call's synchronisation: where the call's `due` records go (the session's list behind the `have` handed out, a peek's own array), and their copy
    // A session that never had k > 0 (dev null) keeps no list: its pushes do no work here, and read hands out off-records for the ids the list does not reach.
    int32_t enqueue(int have, int due, bool peek, vox_token_alts** dst, hipStream_t s) {
        if (peek) { peeked.assign((size_t)due, off()); *dst = peeked.data(); }
        else if (!dev) { peeked.clear(); *dst = nullptr; return VOX_OK; }
        else { peeked.clear(); host.resize((size_t)have + due, off()); *dst = host.data() + have; }
        if (k > 0 && due > 0) HIPCHK(hipMemcpyAsync(*dst, dev + have, (size_t)due * sizeof(TokenAlts), hipMemcpyDeviceToHost, s));
        return VOX_OK;
    }
    void settle(int due, vox_token_alts* dst) const { for (int i = 0; k == 0 && dst && i < due; i++) dst[i] = off(); }      // behind it: a call that ran with alternatives off
    int32_t read(int have, int32_t first_id, int32_t n, vox_token_alts* out) const {
        ARGCHK(first_id >= 0 && n >= 0 && (int64_t)first_id + n <= have, "%d ids from %d on: %d handed out", n, first_id, have);
        ARGCHK(out || n == 0, "null output");
        for (int i = 0; i < n; i++) out[i] = (size_t)(first_id + i) < host.size() ? host[(size_t)(first_id + i)] : off();
        return VOX_OK;
    }
    int32_t read_peeked(vox_token_alts* out, int32_t out_cap, int32_t* n) const {
        ARGCHK(n, "null argument"); ARGCHK(out_cap >= 0 && (size_t)out_cap >= peeked.size(), "capacity %d for the %zu records of the last peek", out_cap, peeked.size());
        ARGCHK(out || peeked.empty(), "null output");
        if (!peeked.empty()) std::memcpy(out, peeked.data(), peeked.size() * sizeof(vox_token_alts));
        *n = (int32_t)peeked.size();
        return VOX_OK;
    }
};
// A session's levels (vox_stream_set_levels; DESIGN.md section 8, "Levels"): ScoreState's twin for the 8-byte records stream_level_kernel writes in front of a tick's
// mel launch.  An engine hand-off timeout repeats decode steps, never a tick (stream_settle comes back through stream_decode_step alone), so level records are never
// computed again.  A peek's tail writes its records behind the session's position and hands none out: the host list is the session's own.  A session that never had
// levels on (dev null) keeps no list.
static_assert(sizeof(vox_tick_level) == 8 && sizeof(TickLevel) == sizeof(vox_tick_level), "vox_tick_level is TickLevel");
struct LevelState {
    bool on = false; TickLevel* dev = nullptr; int cap = 0;
    std::vector<vox_tick_level> host;
    size_t bytes() const { return dev ? (size_t)cap * sizeof(TickLevel) : 0; }
    static vox_tick_level off() { return vox_tick_level{NAN, NAN}; }
    int32_t alloc(int max_pos, const char* whose) {      // the first set(1)
        if (dev) return VOX_OK;
        if (hipMalloc((void**)&dev, (size_t)(max_pos + 2) * sizeof(TickLevel)) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of %s level records failed", whose); }
        cap = max_pos + 2; return VOX_OK;
    }
    int32_t grow(int rows, hipStream_t s) { return list_grow((void**)&dev, &cap, rows, sizeof(TickLevel), s); }      // as ScoreState::grow
    void restart() { host.clear(); }      // create / reset: the list starts over, the flag stays
    // in front of the call's synchronisation: the call's `due` records behind the `have` handed out go to the session's list (a peek: nowhere); off: the records that say so
    int32_t enqueue(int have, int due, bool peek, hipStream_t s) {
        if (peek || !dev) return VOX_OK;
        host.resize((size_t)have + due, off());
        if (on && due > 0) HIPCHK(hipMemcpyAsync(host.data() + have, dev + have, (size_t)due * sizeof(TickLevel), hipMemcpyDeviceToHost, s));
        return VOX_OK;
    }
    int32_t read(int have, int32_t first_id, int32_t n, vox_tick_level* out) const {
        ARGCHK(on, "levels are off (vox_stream_set_levels)");
        ARGCHK(first_id >= 0 && n >= 0 && (int64_t)first_id + n <= have, "%d ids from %d on: %d handed out", n, first_id, have);
        ARGCHK(out || n == 0, "null output");
        for (int i = 0; i < n; i++) out[i] = (size_t)(first_id + i) < host.size() ? host[(size_t)(first_id + i)] : off();
        return VOX_OK;
    }
    // the end-of-speech hint: the trailing records of the `have` ids handed out whose peak < peak_below; a NaN record (a comparison with it is false) ends the run
    int32_t quiet(int have, float peak_below, int32_t* ticks) const {
        ARGCHK(ticks, "null argument"); ARGCHK(std::isfinite(peak_below) && peak_below > 0.0f, "peak_below must be finite and > 0");
        ARGCHK(on, "levels are off (vox_stream_set_levels)");
        int n = 0;
        for (int k = have - 1; k >= 0 && (size_t)k < host.size() && host[(size_t)k].peak < peak_below; k--) n++;
        *ticks = n; return VOX_OK;
    }
};
// One session's share of one call's hand-back -- a solo stream's push / finish / peek, a member's entry of a group's advance / peek: the call's `due` ids from the
// session's device token array into the caller's out_ids, their records into the session's own list or, in a peek, into the caller's array (null: none wanted); their
// alternatives records into the session's list or, in a peek, into the array the session keeps for vox_stream_peeked_alternatives.
namespace {
struct SessionOut {
    FeedState* feed; ScoreState* sc; AltsState* al; LevelState* lv; const int* tokens; int32_t* out_ids; int due;
    bool peek; vox_token_score* peek_scores;      // a peek's records never enter the session's list, and ids_out stays
    vox_token_score* dst = nullptr; vox_token_alts* adst = nullptr;
    int32_t enqueue(hipStream_t s) {      // in front of the call's synchronisation: the records travel with the ids
        const int have = feed->ids_out;
        if (due > 0) HIPCHK(hipMemcpyAsync(out_ids, tokens + VOX_PREFIX_TOKENS + have, (size_t)due * 4, hipMemcpyDeviceToHost, s));
        if (peek) dst = peek_scores; else { sc->host.resize((size_t)have + due); dst = sc->host.data() + have; }
        VOXCHK(sc->enqueue(have, due, dst, s));
        VOXCHK(lv->enqueue(have, due, peek, s));
        return al->enqueue(have, due, peek, &adst, s);
    }
    void settle() { sc->settle(due, out_ids, dst); al->settle(due, adst); if (!peek) feed->ids_out += due; }      // behind it
};
}  // namespace
struct DecPlanes { float *k = nullptr, *v = nullptr; int rows = 0; size_t stride = 0; };      // a decoder cache's planes: what a cache that grew inside a peek leaves behind
struct KeepArea { float* p = nullptr; size_t floats = 0; };      // the ring keep's save area (keep_reserve): allocated at the first peek, counted in its owner's `bytes`
struct vox_stream {
    vox_model* m = nullptr; vox_ctx* ctx = nullptr;
    std::vector<float> t_embed; float gain = 1.0f;
    int cap = 0, max_pos = 0, RC = 0, PC = 0; long left = 0;
    float *kring = nullptr, *vring = nullptr; size_t ring_layer = 0;      // encoder K / V ring: [enc_layers][enc_heads][cap][hd]
    vox_cache* dec = nullptr;                                             // decoder cache (grows from ENGINE_MAX_ROWS rows by doubling, up to max_pos)
    float *samples = nullptr, *audio_keep = nullptr, *ws = nullptr;
    int *tokens = nullptr, *state = nullptr;
    StreamMember* d_mem = nullptr; int* d_order = nullptr;      // the round of one: this stream's descriptor and the order {0} (one allocation)
    MelTables mel{};
    FeedState feed;                    // the session's host mirror (rate, rings' fill, position, ids handed out); feed.At is the stream's OWN block matrix (freed with it)
    int16_t* s16_stage = nullptr;      // host 16-bit pushes: STREAM_FEED_CHUNK samples of device staging, allocated at the first one
    int verified_pos = 0, verified_tap_rows = 0; bool eng_unverified = false;
    uint64_t eng_steps = 0, op_steps = 0, verified_eng_steps = 0, verified_op_steps = 0, bytes = 0;
    EngBinding eng;      // the decode engine's layer table for the stream's cache, its argmax partials (256), the pinned host copy of its error word
    float* tap = nullptr; int tap_max = 0, tap_rows = 0;
    ScoreState sc; float* score_row = nullptr;      // scores: the records, and the logits row a scored step writes when no tap row takes it
    AltsState al;                                   // alternatives: the records (a step with them on writes the same row)
    LevelState lv;                                  // levels: the records (stream_level_kernel, in front of a tick's mel launch)
    float *ftap_mel = nullptr, *ftap_conv = nullptr; int ftap_max = 0, ftap_ticks = 0;      // vox_debug_stream_front_tap_*: per tick its 4 R fresh mel frames and its R conv-stem rows
    int h_state[STRM_WORDS]; int h_pos_word = 0;
    // vox_stream_peek: the ring keep's save area; while a peek's ticks run (active), a decoder cache that grows leaves its planes in `old`: the peek puts them back
    struct { KeepArea keep; bool active = false; DecPlanes old; } peek;
    // An ENDLESS session (vox_stream_create_endless; DESIGN.md section 8, "Endless sessions"): max_pos is 2^24, the decoder cache stops growing at ring_rows rows and is a
    // ring from position ring_rows on (dec_limit: where the cache's growth ends -- ring_rows, or a bounded session's max_pos); the position-indexed device lists
    // (tokens, score and alternatives records) start at lists_cap positions and grow by doubling at a verification point.  rope: the session's two device RoPE rings
    // ([rows][cos hd/2 | sin hd/2], rows a power of two), their pinned host images, and the event behind the last copy out of those images.
    bool endless = false; int ring_rows = 0, dec_limit = 0, lists_cap = 0;
    // A BURST stream (vox_stream_create_burst; DESIGN.md section 8, "Bursts"): up to `burst` due ticks of a pass run as one encoder pass of 4 b rows and b decode steps
    // (stream_burst); 1: every tick is stream_tick.  bursts / burst_ticks: the bursts run with b >= 2 and the ticks inside them; single_ticks: the ticks run one by one
    int burst = 1; uint64_t bursts = 0, burst_ticks = 0, single_ticks = 0;
    struct { float *dec = nullptr, *enc = nullptr, *h_dec = nullptr, *h_enc = nullptr; hipEvent_t copied = nullptr; bool pending = false; } rope;
};
static const int STREAM_TAIL_TICKS = 63;            // the most ticks a finish / peek tail of an endless session may run (peek_max_ticks at the session's rate, asserted at create and in every peek)
static const int STREAM_ROPE_DEC_ROWS = 1024;       // rows of an endless session's decoder RoPE ring = the most ticks of one pass; the encoder's ring has reshape_factor times as many
static const int STREAM_POS_LIMIT = 1 << 24;        // an endless session's position limit (31 days)
static bool stream_in_ring(const vox_stream* st) { return st->endless && st->feed.pos >= st->ring_rows; }      // is the next tick's decoder cache row a ring row?

// the buffers of a round of up to n sessions (n = 1: a solo stream's tick), carved from one allocation; returns its size in floats (base may be null).
// A slot's mel halo is padded from 4 R + 3 to 4 R + 4 frames and its conv1 block from 2 R + 1 to 2 R + 2 rows, so that slots lie a whole number of window strides
// apart and each conv is ONE im2col GEMM over all slots (stream_encode_round); h: the decode step's input rows.
// b > 1 (a solo burst stream, n = 1): the buffers of b ticks in one pass -- 16 b + 3 halo frames, 8 b + 1 and 4 b conv rows, 4 b encoder rows, b adapter rows --
// which the sizes of a round of b slots cover
struct StreamWs { float *halo, *c1, *c2, *x, *xn, *qkv, *att, *ffn, *ah, *arow, *h; };
static size_t stream_ws_carve(const vox_model* m, int n, float* base, StreamWs* w, int b = 1) {
    const vox_model_cfg& c = m->cfg; const size_t R = (size_t)c.reshape_factor, D = (size_t)c.enc_dim, QD = (size_t)c.enc_heads * c.enc_head_dim, N = (size_t)n * (size_t)b;
    StreamWs t; if (!w) w = &t;
    size_t o = 0; auto take = [&](float*& q, size_t k) { q = base ? base + o : nullptr; o += (k + 63) / 64 * 64; };      // (256-byte pieces)
    take(w->halo, N * (4 * R + 4) * c.n_mels); take(w->c1, N * (2 * R + 2) * D); take(w->c2, N * (R + 1) * D); take(w->x, N * R * D); take(w->xn, N * R * D);
    take(w->qkv, N * R * QD * 3); take(w->att, N * R * QD); take(w->ffn, N * R * c.enc_ffn); take(w->ah, N * m->ad0.w.N); take(w->arow, N * c.dec_dim); take(w->h, N * c.dec_dim);
    return o;
}

static int32_t stream_dec_alloc(vox_stream* st, int rows) {      // a fresh decoder cache of `rows` rows (the old one is freed)
    if (st->dec && st->dec->max_seq == rows) return VOX_OK;
    if (st->dec) { HIPCHK(hipStreamSynchronize(st->ctx->stream)); cache_release(st->dec); }
    return cache_alloc(st->m, rows, &st->dec);
}
// the cache is full and the session may go on: twice the rows (at most max_pos), the rows so far copied over.  Happens at a position, not at a push: cut-independent.
// (a new generation: the engine's layer table for the planes so far is stale)
static void dec_set_planes(vox_cache* kc, const DecPlanes& p) { cache_unregister(kc); kc->k = p.k; kc->v = p.v; kc->max_seq = p.rows; kc->layer_stride = p.stride; cache_register(kc); }
// `leave`: where the old planes stay (a peek undoes the growth); null: they are freed
static int32_t stream_dec_grow(vox_stream* st, DecPlanes* leave) {
    vox_model* m = st->m; const vox_model_cfg& c = m->cfg; hipStream_t s = st->ctx->stream; vox_cache* kc = st->dec;
    const int old = kc->max_seq, rows = std::min(st->dec_limit, 2 * old), hd = c.dec_head_dim;
    ARGCHK(rows > old, "internal: decoder cache of %d rows cannot grow", old);
    const size_t planes = (size_t)c.dec_layers * c.dec_kv_heads, nb = planes * rows * hd * 4;
    float *nk = nullptr, *nv = nullptr;
    if (hipMalloc((void**)&nk, nb) != hipSuccess || hipMalloc((void**)&nv, nb) != hipSuccess) { (void)hipGetLastError(); if (nk) (void)hipFree(nk); return fail(VOX_ERR_HIP, "hipMalloc of a %d-row decoder cache failed", rows); }
    HIPCHK(hipMemsetAsync(nk, 0, nb, s)); HIPCHK(hipMemsetAsync(nv, 0, nb, s));
    HIPCHK(hipMemcpy2DAsync(nk, (size_t)rows * hd * 4, kc->k, (size_t)old * hd * 4, (size_t)old * hd * 4, planes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpy2DAsync(nv, (size_t)rows * hd * 4, kc->v, (size_t)old * hd * 4, (size_t)old * hd * 4, planes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (leave) {
        if (leave->k) { (void)hipFree(nk); (void)hipFree(nv); return fail(VOX_ERR_INVALID, "internal: the decoder cache grew twice inside one peek"); }
        *leave = DecPlanes{kc->k, kc->v, old, kc->layer_stride};
    } else { (void)hipFree(kc->k); (void)hipFree(kc->v); }
    dec_set_planes(kc, DecPlanes{nk, nv, rows, (size_t)c.dec_kv_heads * rows * hd});
    return VOX_OK;
}
// the growth undone: the planes a peek's tail left in `old` go back (nothing in flight: the peek has synchronised), the grown ones are freed
static void stream_dec_ungrow(vox_stream* st, DecPlanes* old) {
    if (old->k) { (void)hipFree(st->dec->k); (void)hipFree(st->dec->v); dec_set_planes(st->dec, *old); *old = DecPlanes{}; }
}

// the state after create / reset of a session (a solo stream, a group's member): the prefix state of its t_embed (built here when the model does not hold it, whatever
// vox_model_set_prefix_cache says -- the model's own setting is restored) copied into the session's ring, its decoder cache rows (`dec`: a cache, or a view of a slab's
// slice), its tokens and its state block; the session does not look at the model's copy again.  `then`: what the caller enqueues behind the copies; ONE synchronisation.
template <class Then>
static int32_t stream_seed(vox_model* m, const float* t_embed, int RC, int PC, int cap, float* kring, float* vring, vox_cache* dec, int* tokens, int* state, int* h_state, Then then) {
    const vox_model_cfg& c = m->cfg; hipStream_t s = m->ctx->stream; PrefixState& P = m->pfx;
    const bool was_on = P.on; P.on = true;
    int32_t r = prefix_build(m, t_embed);
    if (r == VOX_OK && !(P.enc_built && P.dec_built && P.RC == RC && P.PC == PC)) r = fail(VOX_ERR_HIP, "the prefix state a stream starts from could not be built");
    auto body = [&]() -> int32_t {
        HIPCHK(launch_stream_ring_init(P.enc_kv, c.enc_layers, RC, c.enc_heads, c.enc_head_dim, cap, kring, vring, s));
        if (dec) VOXCHK(prefix_rows_into(m, dec, s));      // (null: `then` places the rows -- a paged group's member)
        VOXCHK(then());
        HIPCHK(prefix_tokens_enqueue(tokens, s));
        std::memset(h_state, 0, sizeof(int) * STRM_WORDS);
        h_state[STRM_POS] = PC; h_state[STRM_ENC_POS] = RC; h_state[STRM_FRAME] = 4 * RC; h_state[STRM_HEAD] = RC % cap;
        HIPCHK(hipMemcpyAsync(state, h_state, sizeof(int) * STRM_WORDS, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return VOX_OK;
    };
    if (r == VOX_OK) r = body();
    if (!was_on) { (void)hipStreamSynchronize(s); prefix_release(m); P.on = false; }
    return r;
}
static int32_t stream_load_initial(vox_stream* st) {
    vox_model* m = st->m;
    VOXCHK(stream_dec_alloc(st, std::min(st->dec_limit, ENGINE_MAX_ROWS)));
    // the engine's view of THIS cache, in the stream's own binding: no table is rebuilt (and nothing synchronised) when streams, piecewise and offline callers alternate;
    // uploaded behind the seed's copies and in front of its synchronisation, so that the first step finds its cache bound
    VOXCHK(stream_seed(m, st->t_embed.data(), st->RC, st->PC, st->cap, st->kring, st->vring, st->dec, st->tokens, st->state, st->h_state,
                       [&]() -> int32_t { HIPCHK(engine_tab_enqueue(m, st->eng, st->dec)); return VOX_OK; }));
    st->feed.restart(st->PC); st->verified_pos = st->PC; st->eng_unverified = false;
    st->eng_steps = st->op_steps = st->verified_eng_steps = st->verified_op_steps = 0; st->tap_rows = st->verified_tap_rows = 0; st->ftap_ticks = 0;
    st->bursts = st->burst_ticks = st->single_ticks = 0;
    st->sc.host.clear(); st->al.restart(); st->lv.restart();      // the utterance's records start over; the flags and k stay
    return VOX_OK;
}

static void stream_release(vox_stream* st) {
    if (!st) return;
    (void)hipSetDevice(st->ctx->device); (void)hipStreamSynchronize(st->ctx->stream);      // never dereferences st->m: a stream may not outlive its model, but freeing it late must not crash
    cache_release(st->dec);
    for (void* p : {(void*)st->kring, (void*)st->vring, (void*)st->samples, (void*)st->audio_keep, (void*)st->ws, (void*)st->tokens, (void*)st->state, (void*)st->tap, (void*)st->ftap_mel, (void*)st->ftap_conv,
                    (void*)st->feed.At, (void*)st->feed.in_ring, (void*)st->s16_stage, (void*)st->d_mem, (void*)st->sc.dev, (void*)st->score_row, (void*)st->al.dev, (void*)st->lv.dev,
                    (void*)st->peek.keep.p, (void*)st->peek.old.k, (void*)st->peek.old.v, (void*)st->rope.dec, (void*)st->rope.enc}) if (p) (void)hipFree(p);
    if (st->rope.h_dec) (void)hipHostFree(st->rope.h_dec); if (st->rope.h_enc) (void)hipHostFree(st->rope.h_enc);
    if (st->rope.copied) (void)hipEventDestroy(st->rope.copied);
    binding_release(st->eng);
    delete st;
}

// what create checks about the model and the two sizes, for a solo stream and for a group: the prefix bounds, the ring capacity, the position limit
struct StreamGeom { int RC = 0, PC = 0, cap = 0, max_pos = 0; long left = 0; };
// burst: a solo stream's burst_ticks B (1: none) -- a burst appends 4 B rows in one launch, the ring holds window + 4 B rows and more
static int32_t stream_geometry(vox_model* m, int32_t enc_capacity_rows, int32_t max_positions, int default_positions, StreamGeom* g, int burst = 1) {
    const vox_model_cfg& c = m->cfg;
    if (!m->is_q4) return fail(VOX_ERR_UNSUPPORTED, "live streaming sessions serve Q4 (GGUF) models");
    int RC, PC; prefix_bounds(m, &RC, &PC);
    ARGCHK(RC > 0 && c.reshape_factor == 4 && PC == VOX_PREFIX_TOKENS - 1, "this model geometry has no prefix state for a stream to start from");
    if (!m->conv1_g.qs || !m->conv2_g.qs) return fail(VOX_ERR_UNSUPPORTED, "the stream's conv stem runs as im2col GEMMs: 3 n_mels and 3 enc_dim must be multiples of 128");
    ARGCHK(c.enc_window + 1 <= 1024, "encoder window %d exceeds the stream attention's 1023 keys", c.enc_window);
    int cap = enc_capacity_rows; if (cap == 0) cap = (std::max(c.enc_window + 4 * burst + 4, RC) + 63) / 64 * 64;      // a ring needs no slack: anything above window + 4 is exact
    if (burst > 1) ARGCHK(cap > c.enc_window + 4 * burst, "encoder ring capacity %d must exceed the sliding window + 4 burst_ticks (%d + 4 x %d = %d)", cap, c.enc_window, burst, c.enc_window + 4 * burst);
    ARGCHK(cap > c.enc_window + 4 && cap >= RC, "encoder ring capacity %d must exceed the sliding window + 4 (%d)", cap, c.enc_window + 4);
    const int pos_limit = std::min(m->dec_rope_len, (1 << 16) / c.reshape_factor);      // the decoder RoPE table and the 65 536-position streaming encoder table end together
    int maxp = max_positions; if (maxp == 0) maxp = std::min(pos_limit, default_positions);
    ARGCHK(maxp > VOX_PREFIX_TOKENS && maxp <= pos_limit, "max_positions %d out of range (%d..%d)", maxp, VOX_PREFIX_TOKENS + 1, pos_limit);
    g->RC = RC; g->PC = PC; g->cap = cap; g->max_pos = maxp;
    { vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc); g->left = (long)pad_left(&pc); }
    return VOX_OK;
}
// sample_rate 16000: the 16 kHz stream, nothing more; any other rate: + the input ring and the stream's own block matrix
// endless: max_positions is ignored (the limit is 2^24); dec_ring_rows: the decoder ring's rows (0: the default), checked here
static int32_t stream_create(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, uint32_t sample_rate, vox_stream** out,
                             bool endless = false, int32_t dec_ring_rows = 0, int32_t burst = 1) {
    ARGCHK(m && t_embed && out, "null argument"); ARGCHK(std::isfinite(gain), "gain is not finite"); ARGCHK(sample_rate > 0, "bad sample rate 0");
    ARGCHK(burst >= 1 && burst <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst, VOX_STREAM_BURST_MAX);
    VOXCHK(ctx_bind(m->ctx));
    ResamplePlan rp; size_t rs_bytes = 0; int in_ring_n = 0;
    if (sample_rate != 16000) VOXCHK(stream_rate_plan(sample_rate, &rp, &rs_bytes, &in_ring_n));
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx;
    StreamGeom g; VOXCHK(stream_geometry(m, enc_capacity_rows, endless ? 0 : max_positions, INT32_MAX, &g, burst));
    int ring_rows = 0;
    if (endless) {
        // the ring holds a window, the position itself and the rows a finish / peek tail may overwrite ahead of the session: window + 1 + TAIL.  TAIL bounds
        // peek_max_ticks -- vox_stream_peek_ids' arithmetic: the backlog of the rate's unfinished block + the right pad -- at this session's rate
        const int need = c.dec_window + 1 + STREAM_TAIL_TICKS;
        FeedState f; f.sr = sample_rate; f.rp = rp;
        int T; VOXCHK(peek_max_ticks(f, c.reshape_factor, 0, "", &T));
        if (T > STREAM_TAIL_TICKS) return fail(VOX_ERR_UNSUPPORTED, "an endless stream at %u Hz: a finish may run %d ticks, the decoder ring's slack covers %d", sample_rate, T, STREAM_TAIL_TICKS);
        ARGCHK(c.dec_window >= 0, "an endless session needs a sliding decoder window");
        ring_rows = dec_ring_rows ? dec_ring_rows : (need + 63) / 64 * 64;
        ARGCHK(ring_rows >= need, "dec_ring_rows %d: the decoder ring needs at least %d rows (dec_window %d + 1 + %d for a finish / peek tail)", dec_ring_rows, need, c.dec_window, STREAM_TAIL_TICKS);
        const int most = std::min(m->dec_rope_len, ROPE_ENC_STREAM_TABLE_LEN / c.reshape_factor);
        ARGCHK(ring_rows <= most, "dec_ring_rows %d: at most %d (up to the wrap the session reads the load-time RoPE tables)", ring_rows, most);
    }
    VOXCHK(enc_stream_rope_ensure(m));
    vox_stream* st = new vox_stream(); st->m = m; st->ctx = cx; st->t_embed.assign(t_embed, t_embed + c.dec_dim); st->gain = gain; st->cap = g.cap; st->max_pos = g.max_pos; st->RC = g.RC; st->PC = g.PC;
    st->feed.sr = sample_rate; st->feed.rp = rp; st->feed.in_ring_n = in_ring_n; st->left = g.left;
    st->endless = endless; st->ring_rows = ring_rows; st->dec_limit = endless ? ring_rows : g.max_pos; if (endless) st->max_pos = STREAM_POS_LIMIT;
    st->lists_cap = endless ? ring_rows : g.max_pos; st->burst = burst;
    const int DD = c.dec_dim, maxp = st->lists_cap;
    st->ring_layer = (size_t)c.enc_heads * g.cap * c.enc_head_dim;
    const size_t ring_b = (size_t)c.enc_layers * st->ring_layer * 4, keep_b = (size_t)STREAM_KEEP_ROWS * DD * 4, ws_b = stream_ws_carve(m, 1, nullptr, nullptr, burst) * 4;
    hipError_t e = hipSuccess;
    auto A = [&](void** q, size_t n) { if (e == hipSuccess) { e = hipMalloc(q, n); if (e == hipSuccess) st->bytes += n; } };
    A((void**)&st->kring, ring_b); A((void**)&st->vring, ring_b); A((void**)&st->samples, (size_t)STREAM_SAMPLE_RING * 4); A((void**)&st->audio_keep, keep_b);
    A((void**)&st->ws, ws_b); A((void**)&st->tokens, (size_t)(maxp + 2) * 4); A((void**)&st->state, sizeof(int) * STRM_WORDS); A((void**)&st->d_mem, sizeof(StreamMember) + 16);
    if (e == hipSuccess) e = binding_alloc(m, st->eng, &st->bytes);      // (here, not at the first step: the footprint a stream reports does not depend on what it has done)
    if (in_ring_n) A((void**)&st->feed.in_ring, (size_t)in_ring_n * 4);
    if (endless) {      // the RoPE rings and their pinned host images (stream_rope_refill)
        const size_t db = (size_t)STREAM_ROPE_DEC_ROWS * c.dec_head_dim * 4, eb = (size_t)STREAM_ROPE_DEC_ROWS * c.reshape_factor * c.enc_head_dim * 4;
        A((void**)&st->rope.dec, db); A((void**)&st->rope.enc, eb);
        if (e == hipSuccess) e = hipHostMalloc((void**)&st->rope.h_dec, db, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&st->rope.h_enc, eb, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st->rope.copied, hipEventDisableTiming);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); stream_release(st); return fail(VOX_ERR_HIP, "allocating the stream's device state failed: %s", hipGetErrorString(e)); }
    st->d_order = reinterpret_cast<int*>(st->d_mem + 1);
    struct { StreamMember me; int order[4]; } desc{};      // the stream's descriptor never changes; uploaded behind stream_load_initial's synchronisation at the latest
    desc.me.samples = st->samples; desc.me.gain = gain; desc.me.state = st->state; desc.me.kring = st->kring; desc.me.vring = st->vring; desc.me.tokens = st->tokens;
    int32_t r = ctx_mel_tables(cx, &st->mel);
    if (r == VOX_OK && hipMemsetAsync(st->samples, 0, (size_t)STREAM_SAMPLE_RING * 4, cx->stream) != hipSuccess) r = fail(VOX_ERR_HIP, "hipMemsetAsync failed");
    if (r == VOX_OK && hipMemsetAsync(st->ws, 0, ws_b, cx->stream) != hipSuccess) r = fail(VOX_ERR_HIP, "hipMemsetAsync failed");      // (the pad frame and pad row are read, their products are not)
    if (r == VOX_OK && hipMemcpyAsync(st->d_mem, &desc, sizeof(StreamMember) + 16, hipMemcpyHostToDevice, cx->stream) != hipSuccess) r = fail(VOX_ERR_HIP, "hipMemcpyAsync failed");
    if (r == VOX_OK && in_ring_n) { r = resample_matrix_build(cx, rp, rs_bytes, &st->feed.At); if (r == VOX_OK) st->bytes += rs_bytes; }
    if (r == VOX_OK) r = stream_load_initial(st);
    if (r != VOX_OK) { (void)hipStreamSynchronize(cx->stream); stream_release(st); return r; }
    *out = st; return VOX_OK;
}
extern "C" int32_t vox_stream_create(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, vox_stream** out) {
    return stream_create(m, t_embed, gain, enc_capacity_rows, max_positions, 16000, out);
}
extern "C" int32_t vox_stream_create_rate(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, uint32_t sample_rate, vox_stream** out) {
    ARGCHK(sample_rate > 0, "bad sample rate 0");
    return stream_create(m, t_embed, gain, enc_capacity_rows, max_positions, sample_rate, out);
}
extern "C" int32_t vox_stream_create_endless(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t dec_ring_rows, uint32_t sample_rate, vox_stream** out) {
    ARGCHK(m && t_embed && out, "null argument"); ARGCHK(sample_rate > 0, "bad sample rate 0"); ARGCHK(dec_ring_rows >= 0, "dec_ring_rows %d (0: the default)", dec_ring_rows);
    return stream_create(m, t_embed, gain, enc_capacity_rows, 0, sample_rate, out, true, dec_ring_rows);
}
extern "C" int32_t vox_stream_create_burst(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, uint32_t sample_rate, int32_t endless,
                                           int32_t dec_ring_rows, int32_t burst_ticks, vox_stream** out) {
    ARGCHK(m && t_embed && out, "null argument"); ARGCHK(sample_rate > 0, "bad sample rate 0"); ARGCHK(endless == 0 || endless == 1, "endless must be 0 or 1");
    ARGCHK(burst_ticks >= 1 && burst_ticks <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst_ticks, VOX_STREAM_BURST_MAX);
    ARGCHK(dec_ring_rows >= 0 && (endless || dec_ring_rows == 0), "dec_ring_rows %d (0: the default; an endless session's alone)", dec_ring_rows);
    return stream_create(m, t_embed, gain, enc_capacity_rows, endless ? 0 : max_positions, sample_rate, out, endless != 0, dec_ring_rows, burst_ticks);
}
extern "C" int32_t vox_stream_burst_info(const vox_stream* st, int64_t out[4]) {
    ARGCHK(st && out, "null argument");
    out[0] = st->burst; out[1] = (int64_t)st->bursts; out[2] = (int64_t)st->burst_ticks; out[3] = (int64_t)st->single_ticks;
    return VOX_OK;
}
extern "C" int32_t vox_stream_free(vox_stream* st) { stream_release(st); return VOX_OK; }
extern "C" int32_t vox_stream_reset(vox_stream* st) {
    ARGCHK(st, "null stream"); VOXCHK(ctx_bind(st->ctx));
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    return stream_load_initial(st);
}
// words 0 .. 4 of a session's info: samples pushed, position, ids handed out, encoder rows so far, rows held in its ring
static void feed_info(const FeedState& f, int R, int cap, int64_t* out) { out[0] = f.n_pushed; out[1] = f.pos; out[2] = f.ids_out; out[3] = (int64_t)R * f.pos; out[4] = std::min<int64_t>(out[3], cap); }
extern "C" int32_t vox_stream_info(const vox_stream* st, int64_t out[8]) {
    ARGCHK(st && out, "null argument");
    const int R = st->m->cfg.reshape_factor;
    const uint64_t dec_b = st->dec ? 2 * (uint64_t)st->m->cfg.dec_layers * st->dec->layer_stride * 4 : 0, tap_b = (st->tap ? (uint64_t)st->tap_max * st->m->cfg.vocab * 4 : 0) + (st->ftap_mel ? (uint64_t)st->ftap_max * R * (4 * st->m->cfg.n_mels + st->m->cfg.enc_dim) * 4 : 0);
    feed_info(st->feed, R, st->cap, out);
    out[5] = (int64_t)(st->bytes + dec_b + tap_b); out[6] = (int64_t)st->eng_steps; out[7] = (int64_t)st->op_steps;
    return VOX_OK;
}

// the decode step of a tick: input row in the stream's h buffer, position in the state block.  enc_rows = 0: the re-run of an unverified step (the state's encoder
// words stay).  logits_row: where the step's f32 logits go (the tap), or null.  With scores on, stream_score_kernel follows the advance kernel.
static int32_t stream_decode_step(vox_stream* st, float* h, float* logits_row, int enc_rows) {
    vox_model* m = st->m; hipStream_t s = st->ctx->stream; vox_cache* kc = st->dec;
    if ((st->sc.on || st->al.k > 0) && !logits_row) logits_row = st->score_row;      // a scored step always leaves its logits: in the tap's row, else in the stream's own
    const bool ring = stream_in_ring(st);      // (a ring row: the cache is full at ring_rows rows and stays)
    ARGCHK(kc->len == st->feed.pos && (ring ? kc->max_seq == st->ring_rows : st->feed.pos < kc->max_seq), "internal: stream decoder cache at %d, position %d of %d", kc->len, st->feed.pos, kc->max_seq);
    int* pos_word = st->state + STRM_POS;
    if (!ring && engine_bind(m, st->eng, kc)) {      // one launch: the layers against the stream's cache + final norm + lm_head (argmax partials, logits on request)
        VOXCHK(engine_take_serials(m, 1, s));
        HIPCHK(launch_decode_engine(engine_params(m, st->eng, kc, h, pos_word, 0, logits_row), s));
        HIPCHK(launch_stream_advance(st->eng.part_val, st->eng.part_idx, 256, st->tokens, st->state, enc_rows, 4 * enc_rows, st->cap, s));
        st->eng_steps++; st->eng_unverified = true;
    } else {
        const DecRingStep rs{st->rope.dec, STREAM_ROPE_DEC_ROWS - 1};
        VOXCHK(decoder_step_dev(m, h, kc, pos_word, 0, ring ? &rs : nullptr));
        VOXCHK(lm_head_argmax_dev(m, h, logits_row));
        HIPCHK(launch_stream_advance(m->d_part_val, m->d_part_idx, m->n_parts, st->tokens, st->state, enc_rows, 4 * enc_rows, st->cap, s));
        st->op_steps++;
    }
    // the emitted id's record, behind the advance launch of either path -- and of the re-run's steps, which come through here again
    if (st->sc.on) HIPCHK(launch_stream_score(logits_row, m->cfg.vocab, st->d_mem, st->d_order, 1, VOX_PREFIX_TOKENS, s));
    if (st->al.k > 0) HIPCHK(launch_stream_alts(logits_row, m->cfg.vocab, st->d_mem, st->d_order, 1, VOX_PREFIX_TOKENS, s));
    kc->len = ++st->feed.pos;
    return VOX_OK;
}
static float* stream_tap_row(vox_stream* st) {
    if (!st->tap) return nullptr;
    const int k = st->tap_rows++;
    return k < st->tap_max ? st->tap + (size_t)k * st->m->cfg.vocab : nullptr;
}
// behind the decode-engine steps since the last verification: synchronise, read the engine's error word; a hand-off timeout (the GPU is shared) takes those steps back and
// runs them again on the per-operator launches from the kept adapter rows -- the caller sees ids, not an error (the policy of transcribe_dev; three strikes switch the engine off)
static int32_t stream_verify_enqueue(vox_stream* st) {      // the engine's error word on its way to the pinned host word (lands with the next synchronisation)
    return st->eng_unverified ? engine_err_enqueue(st->m, st->eng.err_word, st->ctx->stream) : VOX_OK;
}
static int32_t stream_settle(vox_stream* st, bool* reran) {      // behind that synchronisation
    vox_model* m = st->m; const vox_model_cfg& c = m->cfg; hipStream_t s = st->ctx->stream;
    if (reran) *reran = false;
    const unsigned e = st->eng_unverified ? st->eng.err_word[0] : 0u;
    st->eng_unverified = false;
    if (e) {
        st->eng.err_word[0] = 0u; VOXCHK(engine_strike(m));
        const int p0 = st->verified_pos, p1 = st->feed.pos;
        fprintf(stderr, "[voxtral_hip] decode engine: %s; the stream's steps %d..%d are decoded again on the per-operator path%s\n",
                engine_timeout_text(e, m->eng_strikes).c_str(), p0, p1 - 1, m->eng_strikes >= 3 ? ", the engine is switched off" : "");
        ARGCHK(p1 - p0 <= STREAM_KEEP_ROWS, "internal: %d unverified stream steps", p1 - p0);
        st->eng_steps = st->verified_eng_steps; st->op_steps = st->verified_op_steps;      // the re-run below counts every step again, on the path it then takes
        st->feed.pos = p0; st->dec->len = p0; st->tap_rows = st->verified_tap_rows; st->h_pos_word = p0;
        HIPCHK(hipMemcpyAsync(st->state + STRM_POS, &st->h_pos_word, 4, hipMemcpyHostToDevice, s));
        VOXCHK(wo_acc_clear(m, s));
        StreamWs w; stream_ws_carve(m, 1, st->ws, &w); float* h = w.h;      // (the tick's buffers are free between ticks)
        EngSuspend off(m);
        int32_t r = VOX_OK;
        for (int p = p0; p < p1 && r == VOX_OK; p++) {
            const hipError_t he = launch_stream_embed_kept(m->tok.w, st->tokens, st->audio_keep, STREAM_KEEP_ROWS, c.dec_dim, st->state, h, s);
            if (he != hipSuccess) { r = fail(VOX_ERR_HIP, "launch_stream_embed_kept failed: %s", hipGetErrorString(he)); break; }
            r = stream_decode_step(st, h, stream_tap_row(st), 0);
        }
        VOXCHK(r);
        HIPCHK(hipStreamSynchronize(s));
        if (reran) *reran = true;
    }
    st->verified_pos = st->feed.pos; st->verified_tap_rows = st->tap_rows; st->verified_eng_steps = st->eng_steps; st->verified_op_steps = st->op_steps;
    return VOX_OK;
}
static int32_t stream_verify(vox_stream* st) {      // inside a long push: before the kept rows run out, before the decoder cache moves
    if (st->eng_unverified) { VOXCHK(stream_verify_enqueue(st)); HIPCHK(hipStreamSynchronize(st->ctx->stream)); }
    return stream_settle(st, nullptr);
}

// The encoder half of a tick for a ROUND of r.n sessions (a solo stream: a round of one): mel -> conv stem -> enc_layers x { RMSNorm, q|k|v, ring attention, wo, RMSNorm,
// w1|w3, w2 } -> final norm -> adapter, every weight matrix in ONE launch for all sessions of the round (4 n rows through q4_linear_dev, which picks the kernel by the row
// count).  Slot z works for session r.order[z] (device arrays); w.arow[z] is its adapter row.  ftap_*: a solo stream's front tap (null: none).
// rope (null: the model's streaming table): a solo endless session's encoder RoPE ring, rows = position & rope_mask (StreamAttnParams::rope_mask)
struct StreamRound { const StreamMember* mem; const int* order; int n, cap; size_t ring_layer; MelTables mel; long left; const float* rope = nullptr; int rope_mask = 0, rope_stride = 0; bool levels = false; };      // rope_stride > 0: an endless group's rings, one per member; levels: some session of the round has levels on
// b > 1 (a solo burst stream's round of one, n == 1): the encoder of b ticks in one pass.  Everything the b ticks would read is there before the first (the pass's
// samples, the state block at the burst's first tick), and tick t's rows are rows 4 t .. of every buffer: 16 b + 3 halo frames, 8 b + 1 and 4 b conv windows, 4 b rows
// through the layers with the burst attention, b adapter rows (w.arow[t]: tick t's).  ftap_*: room for ftap_b of the burst's ticks, in the per-tick layout.
// rg (a burst group's round, group_burst_round): slot z runs rg->host->b[z] <= b ticks.  The front end runs with every slot laid out at the stride of b ticks, the rows
// of the ticks a slot does not run are computed and never read; one pack launch puts each slot's valid R b_z conv rows behind the slots before it, and from there on the
// pass has R rg->ticks rows, slot z's at row R tick0[z] -- the ragged burst attention, rg->ticks adapter rows (w.arow[tick0[z] + t]: tick t of slot z).
struct StreamRagged { const StreamBurstDesc* dev; const StreamBurstDesc* host; int ticks; };      // the round's descriptor on the device and on the host; the sum of its b
static int32_t stream_encode_round(vox_model* m, const StreamWs& w, const StreamRound& r, float* ftap_mel, float* ftap_conv, int b = 1, int ftap_b = 1, const StreamRagged* rg = nullptr) {
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    ARGCHK(b >= 1 && b <= VOX_STREAM_BURST_MAX && (b == 1 || r.n == 1 || rg), "internal: a burst of %d ticks in a round of %d", b, r.n);
    ARGCHK(!rg || (rg->dev && rg->host && rg->ticks >= r.n && rg->ticks <= r.n * b && !ftap_mel), "internal: a ragged round of %d ticks in %d slots of %d", rg ? rg->ticks : 0, r.n, b);
    const int D = c.enc_dim, H = c.enc_heads, hd = c.enc_head_dim, QD = H * hd, F = c.enc_ffn, R = c.reshape_factor, DD = c.dec_dim, Cm = c.n_mels, n = r.n, NT = rg ? rg->ticks : n * b, M = R * NT;
    const int NF = 4 * R * b + 3, HS = NF + 1, C1S = 2 * R * b + 2, C2S = R * b + 1;      // mel frames with the halo (conv row s reads frames 4 s - 3 .. 4 s + 3); the slot strides in frames, conv1 rows, conv rows
    // the level records of every tick of the pass, in front of the mel launch: the state block is the one the pass's first tick finds (nothing has advanced it), and the
    // samples are the ones the mel launch is about to read -- whichever of the two comes first pulls them in for the other.  Behind the mel it would sit between two
    // dependent launches of the encoder's chain for no gain.
    if (r.levels) HIPCHK(launch_stream_level(r.mem, r.order, n, STREAM_SAMPLE_RING - 1, r.left, VOX_PREFIX_TOKENS - 1, b, rg ? rg->dev : nullptr, rg ? rg->host : nullptr, s));
    HIPCHK(launch_stream_mel(r.mem, r.order, n, STREAM_SAMPLE_RING - 1, r.left, r.mel, 3, NF, w.halo, (long)HS * Cm, s));
    // conv stem without padding rows, memsets or a transpose: conv1 row i of a slot is the window of its halo rows [2 i, 2 i + 2], conv row i the window of its conv1 rows
    // [2 i, 2 i + 2].  The slots lie C1S / C2S windows apart, so one GEMM per conv serves them all; its last window of every slot but the last straddles two slots: that
    // row is computed and never read.  The R valid rows per slot are then packed into the 4 n-row encoder input (one slot: they are packed as they are).
    float* conv = n == 1 ? w.x : w.c2;
    { GemmParams g{}; g.w = m->conv1_g; g.x = w.halo; g.x_stride = 2 * Cm; g.M = C1S * n - 1; g.out = w.c1; g.out_stride = D; g.bias = m->conv1_b; HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
    { GemmParams g{}; g.w = m->conv2_g; g.x = w.c1; g.x_stride = 2 * D; g.M = C2S * n - 1; g.out = conv; g.out_stride = D; g.bias = m->conv2_b; HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
    if (n > 1 && rg) HIPCHK(launch_stream_burst_pack(w.c2, C2S, rg->dev, n, R, b, D, w.x, s));
    else if (n > 1) HIPCHK(hipMemcpy2DAsync(w.x, (size_t)R * D * 4, w.c2, (size_t)C2S * D * 4, (size_t)R * D * 4, n, hipMemcpyDeviceToDevice, s));
    if (ftap_mel) {      // the front tap (tests): the tick's fresh frames (halo rows 3 ..) and conv rows, copied on the stream
        HIPCHK(hipMemcpyAsync(ftap_mel, w.halo + (size_t)3 * Cm, (size_t)ftap_b * 4 * R * Cm * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ftap_conv, w.x, (size_t)ftap_b * R * D * 4, hipMemcpyDeviceToDevice, s));
    }
    float *x = w.x, *xn = w.xn;
    for (int l = 0; l < c.enc_layers; l++) {
        const EncLayer& L = m->enc[l];
        HIPCHK(launch_rms_norm(x, D, M, D, L.attn_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, L.wqkv.w, L.wqkv.bias, xn, D, M, w.qkv, 3 * QD));
        StreamAttnParams ap{}; ap.qkv = w.qkv; ap.qkv_stride = 3 * QD; ap.mem = r.mem; ap.order = r.order; ap.n = n; ap.ring_off = (size_t)l * r.ring_layer; ap.cap = r.cap;
        ap.cos_t = m->enc_cos_s; ap.sin_t = m->enc_sin_s; ap.out = w.att;
        if (r.rope) { ap.cos_t = r.rope; ap.sin_t = r.rope + hd / 2; ap.rope_mask = r.rope_mask; ap.rope_stride = r.rope_stride; } ap.out_stride = QD; ap.M = R * b; ap.n_heads = H; ap.window = c.enc_window;
        if (rg) HIPCHK(launch_stream_attn_group_burst(ap, rg->dev, *rg->host, R, hd, s));
        else HIPCHK(b >= 2 ? launch_stream_attn_burst(ap, hd, s) : launch_stream_attn(ap, hd, s));
        VOXCHK(q4_linear_dev(cx, L.wo.w, L.wo.bias, w.att, QD, M, x, D, EPI_RESID, x, D));
        HIPCHK(launch_rms_norm(x, D, M, D, L.ffn_norm, nullptr, c.norm_eps, xn, D, s));
        VOXCHK(q4_linear_dev(cx, L.w13.w, nullptr, xn, D, M, w.ffn, F, EPI_SWIGLU));
        VOXCHK(q4_linear_dev(cx, L.w2.w, L.w2.bias, w.ffn, F, M, x, D, EPI_RESID, x, D));
    }
    HIPCHK(launch_rms_norm(x, D, M, D, m->enc_norm, nullptr, c.norm_eps, xn, D, s));
    VOXCHK(q4_linear_dev(cx, m->ad0.w, nullptr, xn, D * R, NT, w.ah, m->ad0.w.N, EPI_GELU));      // a slot's R rows viewed as one [R D] row (models/adapter.rs:108-122)
    VOXCHK(q4_linear_dev(cx, m->ad2.w, nullptr, w.ah, m->ad0.w.N, NT, w.arow, DD));
    return VOX_OK;
}

// An endless session's position-indexed device lists -- the tokens, and the score and alternatives records it has -- are full: twice the positions (at most the
// session's limit), behind a verification (nothing unverified refers to the old arrays), the descriptor pointed at the new ones behind a synchronisation.  They GROW BY
// DOUBLING and are never trimmed: vox_stream_info[5] counts them as they are.
static int32_t stream_lists_grow(vox_stream* st) {
    hipStream_t s = st->ctx->stream;
    VOXCHK(stream_verify(st));
    const int rows = (int)std::min<int64_t>(2LL * st->lists_cap, st->max_pos);
    ARGCHK(rows > st->lists_cap, "internal: the stream's lists of %d positions cannot grow", st->lists_cap);
    const uint64_t had = st->sc.bytes() + st->al.bytes() + st->lv.bytes();
    int tcap = st->lists_cap + 2;
    VOXCHK(list_grow((void**)&st->tokens, &tcap, rows + 2, 4, s)); st->bytes += (uint64_t)(rows - st->lists_cap) * 4;
    if (st->sc.dev) VOXCHK(st->sc.grow(rows + 2, s));
    if (st->al.dev) VOXCHK(st->al.grow(rows + 2, s));
    if (st->lv.dev) VOXCHK(st->lv.grow(rows + 2, s));
    st->bytes += st->sc.bytes() + st->al.bytes() + st->lv.bytes() - had; st->lists_cap = rows;
    struct { int* tok; TokenScore* sp; int scap; TokenAlts* ap; int acap; } w{st->tokens, st->sc.on ? st->sc.dev : nullptr, st->sc.on ? st->sc.cap : 0, st->al.k > 0 ? st->al.dev : nullptr, st->al.k > 0 ? st->al.cap : 0};
    HIPCHK(hipMemcpyAsync(&st->d_mem->tokens, &w.tok, sizeof w.tok, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(&st->d_mem->scores, &w.sp, sizeof w.sp, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->scores_cap, &w.scap, sizeof w.scap, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(&st->d_mem->alts, &w.ap, sizeof w.ap, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->alts_cap, &w.acap, sizeof w.acap, hipMemcpyHostToDevice, s));
    struct { TickLevel* p; int cap; } lw{st->lv.on ? st->lv.dev : nullptr, st->lv.on ? st->lv.cap : 0};
    HIPCHK(hipMemcpyAsync(&st->d_mem->levels, &lw.p, sizeof lw.p, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->levels_cap, &lw.cap, sizeof lw.cap, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
// An endless session's RoPE rows for the n ticks a pass is about to run from position pos0 (some of them at or past the wrap): decoder rows pos0 .. pos0 + n - 1 into row
// position & mask of the decoder ring, the R n encoder rows of those ticks likewise -- made by rope_rows_fill, the tables' own function, in the rings' pinned host
// images and copied with one hipMemcpyAsync per ring (two where the span wraps), in stream order in front of the pass's ticks.
static int32_t stream_rope_refill(vox_stream* st, int pos0, int n) {
    const vox_model_cfg& c = st->m->cfg; hipStream_t s = st->ctx->stream; const int R = c.reshape_factor;
    ARGCHK(n >= 1 && n <= STREAM_ROPE_DEC_ROWS, "internal: a pass of %d ticks, the RoPE rings hold %d", n, STREAM_ROPE_DEC_ROWS);
    // The host images are pinned, so a copy out of them runs when the stream gets to it, long after hipMemcpyAsync has returned -- and positions one ring length apart
    // share a row.  The images must not be rewritten while the last pass's copy may still be in flight: wait for THAT copy (its event, recorded right behind it), not
    // for the ticks queued behind it.  The host so runs at most one pass ahead of the copies.
    if (st->rope.pending) { HIPCHK(hipEventSynchronize(st->rope.copied)); st->rope.pending = false; }
    auto fill = [&](float* host, float* dev, int rows, int hd, int64_t first, int cnt, int64_t table_len) -> int32_t {
        const int half = hd / 2; const int64_t mask = rows - 1;
        for (int i = 0; i < cnt; i++) { float* row = host + (size_t)((first + i) & mask) * hd; rope_rows_fill(hd, c.rope_theta, first + i, 1, table_len, nullptr, row, row + half); }
        const int r0 = (int)(first & mask), k = std::min(cnt, rows - r0);
        HIPCHK(hipMemcpyAsync(dev + (size_t)r0 * hd, host + (size_t)r0 * hd, (size_t)k * hd * 4, hipMemcpyHostToDevice, s));
        if (cnt > k) HIPCHK(hipMemcpyAsync(dev, host, (size_t)(cnt - k) * hd * 4, hipMemcpyHostToDevice, s));      // the span wrapped
        return VOX_OK;
    };
    VOXCHK(fill(st->rope.h_dec, st->rope.dec, STREAM_ROPE_DEC_ROWS, c.dec_head_dim, pos0, n, ROPE_DEC_TABLE_LEN));
    VOXCHK(fill(st->rope.h_enc, st->rope.enc, STREAM_ROPE_DEC_ROWS * R, c.enc_head_dim, (int64_t)st->RC + (int64_t)R * (pos0 - st->PC), R * n, ROPE_ENC_STREAM_TABLE_LEN));
    HIPCHK(hipEventRecord(st->rope.copied, s)); st->rope.pending = true;
    return VOX_OK;
}

// a solo stream's tick: the round of one, then its own decode half -- the engine launch or the per-operator step, with the kept adapter rows behind the re-run
// what the host does in front of the tick at the session's position, where that position asks for it: a verification, the decoder cache's growth, the lists' growth
static int32_t stream_tick_prepare(vox_stream* st) {
    if (st->feed.pos - st->verified_pos >= STREAM_KEEP_ROWS) VOXCHK(stream_verify(st));      // the kept adapter rows cover the unverified steps
    const bool ring = stream_in_ring(st);      // from the wrap on the cache stays as it is: position p lives at row p % ring_rows
    if (!ring && st->feed.pos >= st->dec->max_seq) { VOXCHK(stream_verify(st)); VOXCHK(stream_dec_grow(st, st->peek.active ? &st->peek.old : nullptr)); }
    if (st->endless && st->feed.pos >= st->lists_cap) VOXCHK(stream_lists_grow(st));      // (a bounded session's lists hold its max_pos positions)
    return VOX_OK;
}
// behind stream_tick_prepare: the nearest position above the session's at whose tick the host acts again (or where the encoder's RoPE source changes) -- no burst spans it
static int64_t stream_next_stop(const vox_stream* st) {
    const int pos = st->feed.pos;
    int64_t stop = (int64_t)st->verified_pos + STREAM_KEEP_ROWS;      // the verification limit
    if (!stream_in_ring(st)) stop = std::min<int64_t>(stop, st->dec->max_seq);      // the decoder cache's growth
    if (st->endless && pos < st->ring_rows) stop = std::min<int64_t>(stop, st->ring_rows);      // the wrap into the ring
    if (st->endless) stop = std::min<int64_t>(stop, st->lists_cap);      // the lists' growth
    return stop;
}
static int32_t stream_tick(vox_stream* st) {
    vox_model* m = st->m; const vox_model_cfg& c = m->cfg; hipStream_t s = st->ctx->stream; const int R = c.reshape_factor;
    VOXCHK(stream_tick_prepare(st));
    const bool ring = stream_in_ring(st);
    StreamWs w; stream_ws_carve(m, 1, st->ws, &w);
    StreamRound r{st->d_mem, st->d_order, 1, st->cap, st->ring_layer, st->mel, st->left}; r.levels = st->lv.on;
    if (ring) { r.rope = st->rope.enc; r.rope_mask = STREAM_ROPE_DEC_ROWS * R - 1; }
    const int k = st->ftap_mel ? st->ftap_ticks++ : 0; const bool ftap = st->ftap_mel && k < st->ftap_max;      // (a re-run repeats decode steps, never a tick)
    VOXCHK(stream_encode_round(m, w, r, ftap ? st->ftap_mel + (size_t)k * 4 * R * c.n_mels : nullptr, ftap ? st->ftap_conv + (size_t)k * R * c.enc_dim : nullptr));
    HIPCHK(launch_stream_embed(m->tok.w, st->tokens, w.arow, st->audio_keep, STREAM_KEEP_ROWS, c.dec_dim, st->state, w.h, s));
    return stream_decode_step(st, w.h, stream_tap_row(st), R);
}
// a burst: b >= 2 ticks of a burst stream's pass as ONE encoder pass of R b rows, then the b decode steps of stream_tick, one by one -- the kept adapter rows, the
// tap rows, the records and the engine's verification are per step, as in a tick.  The caller ran stream_tick_prepare and cut b by stream_burst_len: no position of
// the burst asks for the host.  The encoder reads the state block as the burst's first tick finds it; the b advance launches leave it as b ticks would.
static int32_t stream_burst(vox_stream* st, int b) {
    vox_model* m = st->m; const vox_model_cfg& c = m->cfg; hipStream_t s = st->ctx->stream; const int R = c.reshape_factor;
    ARGCHK(b >= 2 && b <= st->burst && st->feed.pos + b <= stream_next_stop(st), "internal: a burst of %d ticks at position %d (burst_ticks %d, next stop %lld)", b, st->feed.pos, st->burst, (long long)stream_next_stop(st));
    const bool ring = stream_in_ring(st);
    StreamWs w; stream_ws_carve(m, 1, st->ws, &w, st->burst);
    StreamRound r{st->d_mem, st->d_order, 1, st->cap, st->ring_layer, st->mel, st->left}; r.levels = st->lv.on;
    if (ring) { r.rope = st->rope.enc; r.rope_mask = STREAM_ROPE_DEC_ROWS * R - 1; }
    const int k = st->ftap_ticks, fb = st->ftap_mel ? std::max(0, std::min(b, st->ftap_max - k)) : 0;      // the burst's ticks the front tap still has room for
    if (st->ftap_mel) st->ftap_ticks += b;
    VOXCHK(stream_encode_round(m, w, r, fb ? st->ftap_mel + (size_t)k * 4 * R * c.n_mels : nullptr, fb ? st->ftap_conv + (size_t)k * R * c.enc_dim : nullptr, b, fb));
    for (int t = 0; t < b; t++) {
        HIPCHK(launch_stream_embed(m->tok.w, st->tokens, w.arow + (size_t)t * c.dec_dim, st->audio_keep, STREAM_KEEP_ROWS, c.dec_dim, st->state, w.h, s));
        VOXCHK(stream_decode_step(st, w.h, stream_tap_row(st), R));
    }
    st->bursts++; st->burst_ticks += (uint64_t)b;
    return VOX_OK;
}

// what a call appends: f32 or 16-bit samples in host or device memory; p null: zeros (the right pad)
struct StreamSrc { const void* p = nullptr; bool s16 = false; int32_t mem_kind = VOX_MEM_DEVICE; };
// samples [at, at + len) of the source into ring[(w0 + k) & (ring_n - 1)], k < len <= ring_n: f32 and zeros as at most two copies (the ring wraps), 16-bit samples through
// stream_s16_kernel (which wraps by itself), host ones in pieces of the staging buffer
static int32_t ring_write_f32(hipStream_t s, float* ring, int ring_n, int64_t w0, const StreamSrc& src, size_t at, size_t len) {      // f32 samples or zeros
    for (size_t w = 0; w < len;) {      // at most two pieces: the ring wraps
        const size_t off = (size_t)((w0 + (int64_t)w) & (ring_n - 1)), k = std::min(len - w, (size_t)ring_n - off);
        if (!src.p) HIPCHK(hipMemsetAsync(ring + off, 0, k * 4, s));
        else HIPCHK(hipMemcpyAsync(ring + off, (const float*)src.p + at + w, k * 4, src.mem_kind == VOX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        w += k;
    }
    return VOX_OK;
}
static int32_t stream_ring_write(vox_stream* st, float* ring, int ring_n, int64_t w0, const StreamSrc& src, size_t at, size_t len) {
    hipStream_t s = st->ctx->stream;
    if (src.p && src.s16) {
        const int16_t* v = (const int16_t*)src.p + at;
        if (src.mem_kind == VOX_MEM_DEVICE) { HIPCHK(launch_stream_s16(v, (int)len, ring, ring_n - 1, (long)w0, s)); return VOX_OK; }
        if (!st->s16_stage) { HIPCHK(hipMalloc((void**)&st->s16_stage, (size_t)STREAM_FEED_CHUNK * 2)); st->bytes += (size_t)STREAM_FEED_CHUNK * 2; }
        for (size_t w = 0; w < len;) {      // (stream order keeps a piece's conversion ahead of the next piece's upload)
            const size_t k = std::min(len - w, (size_t)STREAM_FEED_CHUNK);
            HIPCHK(hipMemcpyAsync(st->s16_stage, v + w, k * 2, hipMemcpyHostToDevice, s));
            HIPCHK(launch_stream_s16(st->s16_stage, (int)k, ring, ring_n - 1, (long)(w0 + (int64_t)w), s));
            w += k;
        }
        return VOX_OK;
    }
    return ring_write_f32(s, ring, ring_n, w0, src, at, len);
}
// the checks on one entry's own arguments.  `who`: what the message starts with ("" for a solo stream's call, "entry 2: ")
static int32_t entry_check(const char* who, const void* samples, size_t n, const int32_t* out_ids, int32_t cap) {
    ARGCHK(samples || n == 0, "%snull samples", who); ARGCHK(n <= ((size_t)1 << 36), "%spush of %zu samples", who, n);
    ARGCHK(cap >= 0 && (out_ids || cap == 0), "%sbad output buffer", who);
    return VOX_OK;
}
// the save area holds `need` floats from here on; its growth is counted in the owner's `bytes`.  `whose`: "stream", "group"
static int32_t keep_reserve(KeepArea& a, size_t need, uint64_t* bytes, hipStream_t s, const char* whose) {
    if (a.floats >= need) return VOX_OK;
    if (a.p) HIPCHK(hipStreamSynchronize(s));      // the area that goes may be in use
    float* q = nullptr;
    if (hipMalloc((void**)&q, need * 4) != hipSuccess) { (void)hipGetLastError(); return fail(VOX_ERR_HIP, "hipMalloc of the %s's %zu-byte peek save area failed", whose, need * 4); }
    if (a.p) (void)hipFree(a.p);
    *bytes += (need - a.floats) * 4; a.p = q; a.floats = need;
    return VOX_OK;
}
// a peek's ring keep (launch_stream_keep; restore 0 in front of the tail's ticks, 1 in front of the call's synchronisation): slot z saves or puts back the state block
// of session order[z] and the `rows` encoder ring rows its tail writes
static StreamKeepParams ring_keep(const vox_model_cfg& c, const StreamMember* mem, const int* order, int n, int rows, int cap, float* keep) {
    StreamKeepParams kp{}; kp.mem = mem; kp.order = order; kp.n = n; kp.layers = c.enc_layers; kp.n_heads = c.enc_heads; kp.hd = c.enc_head_dim; kp.cap = cap;
    kp.rows = rows; kp.keep = keep; kp.slot_stride = stream_keep_floats(c.enc_layers, c.enc_heads, c.enc_head_dim, rows);
    return kp;
}

// What a push / finish / peek does around its ticks: the stream's own Ada scales, clean accumulators, the passes of its one session -- input into its first ring, the
// resampling launch of a rate stream, the pad, then every tick that became due -- then the ids of the call and their records through SessionOut, around ONE synchronisation.
// keep: the call is a peek (stream_peek, which saved the ring rows and takes the host state back): ONE pass, the ring rows and the state block go back in front of the
// call's synchronisation, the records go to peek_scores (null: nowhere), ids_out stays
static int32_t stream_run(vox_stream* st, const StreamSrc& src, FeedPlan& plan, int32_t* out_ids, int32_t* n_ids, const StreamKeepParams* keep = nullptr, vox_token_score* peek_scores = nullptr) {
    vox_model* m = st->m; hipStream_t s = st->ctx->stream; FeedState& f = st->feed; const bool rate = f.sr != 16000, peek = keep != nullptr;
    const int due = plan.due, R = m->cfg.reshape_factor;
    if (m->pw_pend_rows > 0) VOXCHK(pw_sync(m));      // unverified engine steps of the piecewise surface share the engine's error word: settled first
    VOXCHK(vox_model_set_t_embed(m, st->t_embed.data()));
    if (due > 0) VOXCHK(wo_acc_clear(m, s));
    for (int pass = 0; feed_open(f, plan); pass++) {
        if (peek && pass > 0) return peek_second_pass("the stream");
        const FeedPass q = feed_pass(f, plan, R, st->left, SIZE_MAX);
        if (q.idle()) return fail(VOX_ERR_INVALID, "internal: stream stalled at position %d of %d (%lld of %zu samples at 16 kHz)", f.pos, plan.target, (long long)f.n_written, plan.goal16);
        VOXCHK(stream_ring_write(st, rate ? f.in_ring : st->samples, rate ? f.in_ring_n : STREAM_SAMPLE_RING, q.in_w0, src, q.at, q.n_in));
        if (rate) HIPCHK(launch_stream_resample(f.in_ring, f.in_ring_n - 1, (long)f.in_written, f.At, (int)f.rp.fft_in, (int)f.rp.fft_out, (int)f.rp.delay, st->samples, STREAM_SAMPLE_RING - 1,
                                                (long)q.i0, (int)q.n16, s));
        VOXCHK(ring_write_f32(s, st->samples, STREAM_SAMPLE_RING, q.pad_w0, StreamSrc{}, 0, q.pad));
        if (st->endless && q.ticks > 0 && f.pos + q.ticks > st->ring_rows) VOXCHK(stream_rope_refill(st, f.pos, q.ticks));      // the pass reaches the ring: its RoPE rows first
        for (int t = 0; t < q.ticks;) {      // a burst stream: the pass's ticks in bursts, cut where the host must act between ticks; a burst of 1 is a tick
            int b = 1;
            if (st->burst > 1 && q.ticks - t > 1) { VOXCHK(stream_tick_prepare(st)); b = stream_burst_len(q.ticks - t, st->burst, f.pos, stream_next_stop(st)); }
            if (b >= 2) VOXCHK(stream_burst(st, b)); else { VOXCHK(stream_tick(st)); st->single_ticks++; }
            t += b;
        }
    }
    SessionOut o{&f, &st->sc, &st->al, &st->lv, st->tokens, out_ids, due, peek, peek_scores};
    VOXCHK(stream_verify_enqueue(st));
    bool reran = false;
    for (int round = 0; round < 2; round++) {      // a second time only behind the engine's re-run, which wrote the call's ids (and moved STRM_POS) again
        VOXCHK(o.enqueue(s));
        if (peek) HIPCHK(launch_stream_keep(*keep, 1, s));
        HIPCHK(hipStreamSynchronize(s));      // the call's one synchronisation: ids, their records and the engine's verdict land together
        if (round == 0) VOXCHK(stream_settle(st, &reran));
        if (!reran) break;
    }
    *n_ids = due; o.settle();
    return VOX_OK;
}
// vox_stream_peek behind its checks: finish's ticks, then the session as it was.  The device takes back the encoder ring rows the tail wrote and the state block
// (the ring keep, its restore inside stream_run); the host takes back the feed, what StreamMark holds next to it, and a decoder cache that grew.  Everything else the
// tail wrote lies past the session's position and is written again before it is read.
struct StreamMark { FeedState::Mark feed; int tap_rows, ftap_ticks; uint64_t eng_steps, op_steps, bursts, burst_ticks, single_ticks; };      // (the verified counters are set to the same: stream_peek verifies first)
static int32_t stream_peek(vox_stream* st, FeedPlan& plan, int32_t* out_ids, int32_t* n_ids, vox_token_score* scores) {
    vox_model* m = st->m; const vox_model_cfg& c = m->cfg; hipStream_t s = st->ctx->stream; FeedState& f = st->feed;
    int T; VOXCHK(peek_max_ticks(f, c.reshape_factor, plan.due, "", &T));
    // An endless session past its wrap needs no decoder save: the tail's T ticks overwrite ring rows (pos .. pos + T - 1) % ring_rows, which held positions at most
    // pos + T - 1 - ring_rows < pos - dec_window -- outside the window of every later position.  That is what the ring's TAIL rows of slack buy
    ARGCHK(!st->endless || (T <= STREAM_TAIL_TICKS && st->ring_rows >= c.dec_window + 1 + T), "internal: a peek of %d ticks against a decoder ring with %d rows of slack", T, st->ring_rows - c.dec_window - 1);
    const int rows = std::min(st->cap, c.reshape_factor * T);      // (a function of the stream's rate and capacity: the area is reserved once)
    VOXCHK(keep_reserve(st->peek.keep, stream_keep_floats(c.enc_layers, c.enc_heads, c.enc_head_dim, rows), &st->bytes, s, "stream"));
    if (m->pw_pend_rows > 0) VOXCHK(pw_sync(m));
    VOXCHK(stream_verify(st));      // the kept adapter rows cover the tail alone; verified_* are the session's own from here
    const StreamMark was{f.mark(), st->tap_rows, st->ftap_ticks, st->eng_steps, st->op_steps, st->bursts, st->burst_ticks, st->single_ticks};
    const StreamKeepParams keep = ring_keep(c, st->d_mem, st->d_order, 1, rows, st->cap, st->peek.keep.p);      // the round of one
    HIPCHK(launch_stream_keep(keep, 0, s));
    st->peek.active = true;
    const int32_t r = stream_run(st, StreamSrc{}, plan, out_ids, n_ids, &keep, scores);
    st->peek.active = false;
    if (r != VOX_OK) { (void)launch_stream_keep(keep, 1, s); (void)hipStreamSynchronize(s); st->eng_unverified = false; }      // a failed tail is taken back as well
    stream_dec_ungrow(st, &st->peek.old);      // the tail crossed the cache's rows: engine_bind meets a new generation and rebuilds its table
    f.rewind(was.feed); st->dec->len = st->verified_pos = f.pos;
    st->tap_rows = st->verified_tap_rows = was.tap_rows; st->ftap_ticks = was.ftap_ticks;
    st->eng_steps = st->verified_eng_steps = was.eng_steps; st->op_steps = st->verified_op_steps = was.op_steps;
    st->bursts = was.bursts; st->burst_ticks = was.burst_ticks; st->single_ticks = was.single_ticks;
    return r;
}

// a solo stream's entry -- push, finish, peek: every check, the plan, nothing changed (a refused call can be repeated); then the stream's device
static int32_t stream_enter(vox_stream* st, const void* samples, size_t n, bool finish, int32_t* out_ids, int32_t cap, int32_t* n_ids, FeedPlan* plan) {
    ARGCHK(st && n_ids && (samples || n == 0), "null argument"); VOXCHK(entry_check("", samples, n, out_ids, cap));
    VOXCHK(feed_plan(st->feed, st->m->cfg.reshape_factor, st->left, st->max_pos, n, finish, cap, "the stream", plan));
    return ctx_bind(st->ctx);
}
static int32_t stream_push(vox_stream* st, const void* samples, bool s16, size_t n, int32_t mem_kind, int32_t* out_ids, int32_t cap, int32_t* n_ids) {
    ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    FeedPlan plan; VOXCHK(stream_enter(st, samples, n, false, out_ids, cap, n_ids, &plan));
    st->feed.n_pushed += (int64_t)n;
    StreamSrc src; src.p = samples; src.s16 = s16; src.mem_kind = mem_kind;
    return stream_run(st, src, plan, out_ids, n_ids);
}
extern "C" int32_t vox_stream_push(vox_stream* st, const float* samples, size_t n, int32_t mem_kind, int32_t* out_ids, int32_t cap, int32_t* n_ids) {
    return stream_push(st, samples, false, n, mem_kind, out_ids, cap, n_ids);
}
extern "C" int32_t vox_stream_push_s16(vox_stream* st, const int16_t* samples, size_t n, int32_t mem_kind, int32_t* out_ids, int32_t cap, int32_t* n_ids) {
    return stream_push(st, samples, true, n, mem_kind, out_ids, cap, n_ids);
}
extern "C" int32_t vox_stream_finish(vox_stream* st, int32_t* out_ids, int32_t cap, int32_t* n_ids) {
    FeedPlan plan; VOXCHK(stream_enter(st, nullptr, 0, true, out_ids, cap, n_ids, &plan));
    VOXCHK(stream_run(st, StreamSrc{}, plan, out_ids, n_ids));
    st->feed.finished = true;
    return VOX_OK;
}

extern "C" int32_t vox_stream_peek(vox_stream* st, int32_t* out_ids, int32_t cap, int32_t* n_ids, vox_token_score* scores_or_null) {
    FeedPlan plan; VOXCHK(stream_enter(st, nullptr, 0, true, out_ids, cap, n_ids, &plan));      // finish's refusals, nothing changed
    return stream_peek(st, plan, out_ids, n_ids, scores_or_null);
}

// the stream's own logits row, for the steps of a scored stream (scores or alternatives) that no tap row takes: allocated once
static int32_t stream_own_row(vox_stream* st) {
    if (st->score_row) return VOX_OK;
    const size_t row_b = (size_t)st->m->cfg.vocab * 4;
    if (hipMalloc((void**)&st->score_row, row_b) != hipSuccess) { (void)hipGetLastError(); st->score_row = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of the stream's logits row failed"); }
    st->bytes += row_b;
    return VOX_OK;
}
// scores on / off.  The first on allocates the records and the logits row; the stream's descriptor carries the records' pointer only while scores are on (the kernel's
// own check), uploaded behind a synchronisation: nothing of an earlier call is in flight then
extern "C" int32_t vox_stream_set_scores(vox_stream* st, int32_t on) {
    ARGCHK(st, "null stream"); ARGCHK(on == 0 || on == 1, "on must be 0 or 1"); VOXCHK(ctx_bind(st->ctx));
    hipStream_t s = st->ctx->stream; ScoreState& sc = st->sc;
    if (on) {      // the first on: the records, and the stream's own logits row
        const size_t had = sc.bytes();
        VOXCHK(sc.alloc(st->lists_cap, "the stream's")); st->bytes += sc.bytes() - had;
        VOXCHK(stream_own_row(st));
    }
    HIPCHK(hipStreamSynchronize(s));
    struct { TokenScore* p; int cap; } w{on ? sc.dev : nullptr, on ? sc.cap : 0};
    HIPCHK(hipMemcpyAsync(&st->d_mem->scores, &w.p, sizeof w.p, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->scores_cap, &w.cap, sizeof w.cap, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    sc.on = on != 0;
    return VOX_OK;
}
extern "C" int32_t vox_stream_scores(const vox_stream* st, int32_t first_id, int32_t n, vox_token_score* out) {
    ARGCHK(st, "null stream");
    return st->sc.read(st->feed.ids_out, first_id, n, out);
}

// levels on / off, as scores: the first on allocates the records; the descriptor carries their pointer only while levels are on, uploaded behind a synchronisation
extern "C" int32_t vox_stream_set_levels(vox_stream* st, int32_t on) {
    ARGCHK(st, "null stream"); ARGCHK(on == 0 || on == 1, "on must be 0 or 1"); VOXCHK(ctx_bind(st->ctx));
    hipStream_t s = st->ctx->stream; LevelState& lv = st->lv;
    if (on) { const size_t had = lv.bytes(); VOXCHK(lv.alloc(st->lists_cap, "the stream's")); st->bytes += lv.bytes() - had; }
    HIPCHK(hipStreamSynchronize(s));
    struct { TickLevel* p; int cap; } w{on ? lv.dev : nullptr, on ? lv.cap : 0};
    HIPCHK(hipMemcpyAsync(&st->d_mem->levels, &w.p, sizeof w.p, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->levels_cap, &w.cap, sizeof w.cap, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    lv.on = on != 0;
    return VOX_OK;
}
extern "C" int32_t vox_stream_levels(const vox_stream* st, int32_t first_id, int32_t n, vox_tick_level* out) {
    ARGCHK(st, "null stream");
    return st->lv.read(st->feed.ids_out, first_id, n, out);
}
extern "C" int32_t vox_stream_quiet(const vox_stream* st, float peak_below, int32_t* ticks) {
    ARGCHK(st, "null stream");
    return st->lv.quiet(st->feed.ids_out, peak_below, ticks);
}
// the arithmetic of a record's window (host only): [2560 (k - 1), 2560 k) of the utterance's 16 kHz samples
extern "C" int32_t vox_level_window(int32_t k, int64_t* first_sample, int64_t* end_sample) {
    ARGCHK(first_sample && end_sample, "null argument"); ARGCHK(k >= 0, "record index %d", k);
    *first_sample = (int64_t)LEVEL_TICK * ((int64_t)k - 1); *end_sample = (int64_t)LEVEL_TICK * k;
    return VOX_OK;
}

// alternatives at k (0: off), as scores on / off: the first k > 0 allocates the records and, unless scores did, the logits row; the descriptor carries the records'
// pointer only while k > 0, and the k, uploaded behind a synchronisation
extern "C" int32_t vox_stream_set_alternatives(vox_stream* st, int32_t k) {
    ARGCHK(st, "null stream"); ARGCHK(k >= 0 && k <= VOX_MAX_ALTERNATIVES, "k %d out of range (0..%d)", k, VOX_MAX_ALTERNATIVES); VOXCHK(ctx_bind(st->ctx));
    hipStream_t s = st->ctx->stream; AltsState& al = st->al;
    if (k > 0) {
        const size_t had = al.bytes();
        VOXCHK(al.alloc(st->lists_cap, "the stream's")); st->bytes += al.bytes() - had;
        VOXCHK(stream_own_row(st));
    }
    HIPCHK(hipStreamSynchronize(s));
    struct { TokenAlts* p; int cap, k; } w{k > 0 ? al.dev : nullptr, k > 0 ? al.cap : 0, k};
    HIPCHK(hipMemcpyAsync(&st->d_mem->alts, &w.p, sizeof w.p, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(&st->d_mem->alts_cap, &w.cap, sizeof w.cap, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(&st->d_mem->alts_k, &w.k, sizeof w.k, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    al.k = k;
    return VOX_OK;
}
extern "C" int32_t vox_stream_alternatives(const vox_stream* st, int32_t first_id, int32_t n, vox_token_alts* out) {
    ARGCHK(st, "null stream");
    return st->al.read(st->feed.ids_out, first_id, n, out);
}
extern "C" int32_t vox_stream_peeked_alternatives(const vox_stream* st, vox_token_alts* out, int32_t cap, int32_t* n) {
    ARGCHK(st, "null stream");
    return st->al.read_peeked(out, cap, n);
}

extern "C" int32_t vox_debug_stream_tap_arm(vox_stream* st, int32_t max_rows) {
    ARGCHK(st, "null stream"); ARGCHK(max_rows > 0 && max_rows <= 65536, "max_rows %d out of range (1..65536)", max_rows); VOXCHK(ctx_bind(st->ctx));
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    if (st->tap) { (void)hipFree(st->tap); st->tap = nullptr; }
    HIPCHK(hipMalloc((void**)&st->tap, (size_t)max_rows * st->m->cfg.vocab * 4));
    st->tap_max = max_rows; st->tap_rows = st->verified_tap_rows = 0;
    return VOX_OK;
}
extern "C" int32_t vox_debug_stream_tap_fetch(vox_stream* st, float* out, int32_t* rows) {
    ARGCHK(st && out && rows, "null argument"); ARGCHK(st->tap, "no stream tap to fetch (vox_debug_stream_tap_arm)"); VOXCHK(ctx_bind(st->ctx));
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    const int k = std::min(st->tap_rows, st->tap_max);
    if (k > 0) HIPCHK(hipMemcpy(out, st->tap, (size_t)k * st->m->cfg.vocab * 4, hipMemcpyDeviceToHost));
    *rows = st->tap_rows;
    (void)hipFree(st->tap); st->tap = nullptr; st->tap_max = 0; st->tap_rows = st->verified_tap_rows = 0;
    return VOX_OK;
}
// the rows a peek left BEHIND the tap's position (tests): the tail's logits rows stay in the tap's buffer until the session's own ticks write over them
extern "C" int32_t vox_debug_stream_tap_peeked(vox_stream* st, float* out, int32_t rows) {
    ARGCHK(st && out, "null argument"); ARGCHK(st->tap, "no stream tap armed (vox_debug_stream_tap_arm)"); VOXCHK(ctx_bind(st->ctx));
    ARGCHK(rows >= 0 && st->tap_rows + rows <= st->tap_max, "%d peeked rows behind %d of a tap of %d", rows, st->tap_rows, st->tap_max);
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    if (rows > 0) HIPCHK(hipMemcpy(out, st->tap + (size_t)st->tap_rows * st->m->cfg.vocab, (size_t)rows * st->m->cfg.vocab * 4, hipMemcpyDeviceToHost));
    return VOX_OK;
}

static void stream_front_tap_drop(vox_stream* st) {
    if (st->ftap_mel) (void)hipFree(st->ftap_mel);
    if (st->ftap_conv) (void)hipFree(st->ftap_conv);
    st->ftap_mel = st->ftap_conv = nullptr; st->ftap_max = st->ftap_ticks = 0;
}
extern "C" int32_t vox_debug_stream_front_tap_arm(vox_stream* st, int32_t max_ticks) {
    ARGCHK(st, "null stream"); ARGCHK(max_ticks > 0 && max_ticks <= 65536, "max_ticks %d out of range (1..65536)", max_ticks); VOXCHK(ctx_bind(st->ctx));
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    stream_front_tap_drop(st);
    const vox_model_cfg& c = st->m->cfg; const size_t R = (size_t)c.reshape_factor;
    HIPCHK(hipMalloc((void**)&st->ftap_mel, (size_t)max_ticks * 4 * R * c.n_mels * 4));
    if (hipMalloc((void**)&st->ftap_conv, (size_t)max_ticks * R * c.enc_dim * 4) != hipSuccess) { (void)hipGetLastError(); stream_front_tap_drop(st); return fail(VOX_ERR_HIP, "hipMalloc of the stream front tap failed"); }
    st->ftap_max = max_ticks;
    return VOX_OK;
}
extern "C" int32_t vox_debug_stream_front_tap_fetch(vox_stream* st, float* out_mel, float* out_conv, int32_t* ticks) {
    ARGCHK(st && out_mel && out_conv && ticks, "null argument"); ARGCHK(st->ftap_mel, "no stream front tap to fetch (vox_debug_stream_front_tap_arm)"); VOXCHK(ctx_bind(st->ctx));
    HIPCHK(hipStreamSynchronize(st->ctx->stream));
    const vox_model_cfg& c = st->m->cfg; const size_t R = (size_t)c.reshape_factor, k = (size_t)std::min(st->ftap_ticks, st->ftap_max);
    if (k > 0) { HIPCHK(hipMemcpy(out_mel, st->ftap_mel, k * 4 * R * c.n_mels * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_conv, st->ftap_conv, k * R * c.enc_dim * 4, hipMemcpyDeviceToHost)); }
    *ticks = st->ftap_ticks;
    stream_front_tap_drop(st);
    return VOX_OK;
}

// ------------------------------------------------------------------------------------------------
// Snapshot and resume (vox_stream_snapshot, vox_stream_restore; DESIGN.md section 8, "Snapshot and resume"; the blob's format: vox_snapshot.h).  Between two calls
// nothing of a session is in flight or unverified, so the session IS its device arrays and its host mirror; the blob holds the part of them a later tick can read:
// the K / V rows inside the two windows (launch_snapshot_kv gathers them from, and scatters them into, whatever layout the container has), the two sample rings in
// logical order, the tokens, the host record lists.  The state block is not stored: its words follow from D (STRM_ENC_POS = R D, STRM_FRAME = 4 R D, STRM_TICKS =
// D - PC) and from the target's ring capacity (STRM_HEAD).
// ------------------------------------------------------------------------------------------------
static const size_t SNAP_STAGE_MAX = (size_t)64 << 20;      // a host blob's K / V sections pass through at most this much device staging, in two halves
// the model's fingerprint, computed once: the configuration, the parsed weights' byte count, and a hash of three 4 KB pieces of them (start, middle, end) read back here
static int32_t model_fingerprint(vox_model* m, uint64_t* out) {
    if (!m->snap_fingerprint_set) {
        const uint64_t n = m->arena_primary_bytes ? m->arena_primary_bytes : m->arena_bytes, piece = std::min<uint64_t>(4096, n);
        std::vector<unsigned char> buf((size_t)(3 * piece));
        const uint64_t at[3] = {0, (n - piece) / 2 & ~(uint64_t)15, n - piece};
        HIPCHK(hipStreamSynchronize(m->ctx->stream));
        for (int i = 0; i < 3 && piece; i++) HIPCHK(hipMemcpy(buf.data() + (size_t)i * piece, m->arena + at[i], (size_t)piece, hipMemcpyDeviceToHost));
        m->snap_fingerprint = vox_snap::snap_fingerprint(m->cfg, n, vox_snap::fnv1a(buf.data(), buf.size())); m->snap_fingerprint_set = true;
    }
    *out = m->snap_fingerprint; return VOX_OK;
}
// one stack's K / V sections between a cache (kp: everything but the blob pointers and the planes) and the blob's two sections.  A device blob: one launch straight on
// the caller's buffer.  A host blob: pieces of whole planes through the staging area's halves in turn ([K piece | V piece] each), every piece one launch and two copies,
// all in stream order -- the copy out of a half is queued ahead of the next launch into it.
static int32_t snap_move_stack(hipStream_t s, vox::SnapshotKvParams kp, char* blob_k, char* blob_v, int32_t mem_kind, int restore, float* stage, size_t stage_bytes, int* half) {
    const int rows = kp.hi - kp.lo, all = kp.layers * kp.heads;
    if (rows <= 0) return VOX_OK;
    const size_t plane_b = (size_t)rows * kp.hd * 4;
    if (mem_kind == VOX_MEM_DEVICE) {
        for (int p0 = 0; p0 < all; p0 += 32768) {
            kp.plane0 = p0; kp.n_planes = std::min(32768, all - p0); kp.blob_k = reinterpret_cast<float*>(blob_k + (size_t)p0 * plane_b); kp.blob_v = reinterpret_cast<float*>(blob_v + (size_t)p0 * plane_b);
            HIPCHK(launch_snapshot_kv(kp, restore, s));
        }
        return VOX_OK;
    }
    const size_t half_b = stage_bytes / 2; const int per = (int)std::min<size_t>((size_t)std::min(all, 32768), half_b / 2 / plane_b);
    ARGCHK(stage && per >= 1, "internal: a %zu-byte plane does not fit the snapshot staging area of %zu bytes", plane_b, stage_bytes);
    for (int p0 = 0; p0 < all; p0 += per, *half ^= 1) {
        const int n = std::min(per, all - p0); const size_t piece_b = (size_t)n * plane_b;
        char* hk = reinterpret_cast<char*>(stage) + (size_t)*half * half_b; char* hv = hk + piece_b;
        kp.plane0 = p0; kp.n_planes = n; kp.blob_k = reinterpret_cast<float*>(hk); kp.blob_v = reinterpret_cast<float*>(hv);
        if (restore) {
            HIPCHK(hipMemcpyAsync(hk, blob_k + (size_t)p0 * plane_b, piece_b, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(hv, blob_v + (size_t)p0 * plane_b, piece_b, hipMemcpyHostToDevice, s));
            HIPCHK(launch_snapshot_kv(kp, 1, s));
        } else {
            HIPCHK(launch_snapshot_kv(kp, 0, s));
            HIPCHK(hipMemcpyAsync(blob_k + (size_t)p0 * plane_b, hk, piece_b, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(blob_v + (size_t)p0 * plane_b, hv, piece_b, hipMemcpyDeviceToHost, s));
        }
    }
    return VOX_OK;
}
// the staging a host blob of this header needs: both halves of the larger stack, at most SNAP_STAGE_MAX (a multiple of 64 bytes, so both halves stay 16-byte aligned)
static size_t snap_stage_bytes(const vox_snap::SnapHeader& h) {
    const uint64_t most = 2 * std::max(h.sec_len[vox_snap::SEC_ENC_K], h.sec_len[vox_snap::SEC_DEC_K]);
    return (size_t)((std::min<uint64_t>(2 * most, SNAP_STAGE_MAX) + 63) & ~(uint64_t)63);
}
// What snapshot and restore see of ONE session, whatever holds it -- a solo stream, a member of a slab, paged or endless group: its host mirror and record lists, its
// device arrays, and its two K / V stacks as launch_snapshot_kv addresses them (everything but the rows and the blob pointers).  The container fills it in; the two
// functions below never look at the container again.
struct SnapSession {
    vox_model* m; vox_ctx* ctx; const std::vector<float>* t_embed; FeedState* feed; ScoreState* sc; AltsState* al; LevelState* lv; float gain;
    int* tokens; float* samples; int* state; int* h_state;
    int cap, PC, max_pos;      // its encoder ring's capacity, the prefix positions, its position limit
    vox::SnapshotKvParams enc, dec;
    const char* who;           // the messages' subject: "the stream", "member 3"
};
static void snap_rows(vox::SnapshotKvParams* enc, vox::SnapshotKvParams* dec, const vox_snap::SnapHeader& h) { enc->lo = h.E - h.We; enc->hi = h.E; dec->lo = h.D - h.Wd; dec->hi = h.D; }
// the header of the session as it stands (host arithmetic; token and fingerprint are the caller's)
static void session_snap_header(const SnapSession& ss, vox_snap::SnapHeader* h) {
    using namespace vox_snap;
    const FeedState& f = *ss.feed; const vox_model_cfg& c = ss.m->cfg;
    *h = SnapHeader{}; h->magic = SNAP_MAGIC; h->version = VOX_SNAPSHOT_VERSION;
    h->t_embed_hash = fnv1a(ss.t_embed->data(), ss.t_embed->size() * 4);
    h->gain = ss.gain; h->sample_rate = f.sr; h->n_pushed = f.n_pushed; h->n_written = f.n_written; h->in_written = f.in_written;
    h->D = f.pos; h->E = c.reshape_factor * f.pos; h->ids_out = f.ids_out; h->scores_on = ss.sc->on ? 1 : 0; h->alts_k = ss.al->k;
    SnapShape s; s.D = h->D; s.E = h->E; s.n_written = f.n_written; s.in_samples = f.sr != 16000 ? std::min<int64_t>(f.in_written, f.in_ring_n) : 0;
    s.n_scores = ss.sc->on ? f.ids_out : 0; s.n_alts = ss.al->k > 0 ? f.ids_out : 0;
    h->total_bytes = snap_layout(c, s, h);
}
// the last `n` samples of a ring of ring_n (a power of two) whose next write goes to `end`, in logical order, to dst: at most two copies
static int32_t snap_ring_out(hipStream_t s, const float* ring, int ring_n, int64_t end, size_t n, char* dst, hipMemcpyKind kind) {
    const int64_t first = end - (int64_t)n;
    for (size_t w = 0; w < n;) {
        const size_t off = (size_t)((first + (int64_t)w) & (ring_n - 1)), k = std::min(n - w, (size_t)ring_n - off);
        HIPCHK(hipMemcpyAsync(dst + w * 4, ring + off, k * 4, kind, s)); w += k;
    }
    return VOX_OK;
}
// vox_stream_snapshot / vox_stream_group_snapshot behind the container: nothing of the session is written.  Two synchronisations: the token at D, the finished blob.
static int32_t session_snapshot(const SnapSession& ss, void* blob, size_t cap, size_t* nbytes, int32_t mem_kind) {
    using namespace vox_snap;
    ARGCHK(blob && nbytes, "null argument"); ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    ARGCHK(!ss.feed->finished, "%s is finished: a reset starts its next utterance", ss.who);
    ARGCHK(mem_kind == VOX_MEM_HOST || !(reinterpret_cast<uintptr_t>(blob) & 15), "a device blob must be 16-byte aligned");
    SnapHeader h; session_snap_header(ss, &h);
    ARGCHK(cap >= h.total_bytes, "snapshot: capacity %zu < the %llu bytes of the blob", cap, (unsigned long long)h.total_bytes);
    vox_model* m = ss.m; hipStream_t s = ss.ctx->stream; const bool dev = mem_kind == VOX_MEM_DEVICE; char* b = static_cast<char*>(blob); const FeedState& f = *ss.feed;
    VOXCHK(model_fingerprint(m, &h.fingerprint));
    HIPCHK(hipMemcpyAsync(&h.token, ss.tokens + h.D, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));      // the first of the call's two synchronisations: the token at D (nothing of the session is in flight between calls)
    ARGCHK(h.token >= 0 && h.token < m->cfg.vocab, "internal: %s: token %d at position %d is outside the vocabulary", ss.who, h.token, h.D);
    DevBuf stage; const size_t stage_b = dev ? 0 : snap_stage_bytes(h);
    if (stage_b && hipMalloc(&stage.p, stage_b) != hipSuccess) { (void)hipGetLastError(); stage.p = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of the snapshot's %zu-byte staging area failed", stage_b); }
    const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    auto put = [&](uint64_t off, const void* src, size_t n) -> int32_t {      // host data into the blob (a device blob: read at the call's last synchronisation at the latest)
        if (dev) HIPCHK(hipMemcpyAsync(b + off, src, n, hipMemcpyHostToDevice, s)); else std::memcpy(b + off, src, n);
        return VOX_OK;
    };
    std::vector<vox_token_alts> alts;      // (lives until the call's last synchronisation: a device blob's copy reads it)
    auto body = [&]() -> int32_t {
        for (int i = 0; i < SEC_COUNT; i++) {      // the padding behind every section
            const uint64_t end = h.sec_off[i] + h.sec_len[i], next = i + 1 < SEC_COUNT ? h.sec_off[i + 1] : h.total_bytes;
            if (next > end) { if (dev) HIPCHK(hipMemsetAsync(b + end, 0, (size_t)(next - end), s)); else std::memset(b + end, 0, (size_t)(next - end)); }
        }
        int half = 0; vox::SnapshotKvParams enc = ss.enc, dec = ss.dec; snap_rows(&enc, &dec, h);
        VOXCHK(snap_move_stack(s, enc, b + h.sec_off[SEC_ENC_K], b + h.sec_off[SEC_ENC_V], mem_kind, 0, stage.as<float>(), stage_b, &half));
        VOXCHK(snap_move_stack(s, dec, b + h.sec_off[SEC_DEC_K], b + h.sec_off[SEC_DEC_V], mem_kind, 0, stage.as<float>(), stage_b, &half));
        VOXCHK(snap_ring_out(s, ss.samples, STREAM_SAMPLE_RING, h.n_written, (size_t)(h.sec_len[SEC_SAMPLES] / 4), b + h.sec_off[SEC_SAMPLES], out));
        if (h.sec_len[SEC_IN_SAMPLES]) VOXCHK(snap_ring_out(s, f.in_ring, f.in_ring_n, h.in_written, (size_t)(h.sec_len[SEC_IN_SAMPLES] / 4), b + h.sec_off[SEC_IN_SAMPLES], out));
        HIPCHK(hipMemcpyAsync(b + h.sec_off[SEC_TOKENS], ss.tokens, (size_t)h.sec_len[SEC_TOKENS], out, s));
        if (h.n_scores) {
            ARGCHK(ss.sc->host.size() == (size_t)h.n_scores, "internal: %zu score records for %d ids", ss.sc->host.size(), h.n_scores);
            VOXCHK(put(h.sec_off[SEC_SCORES], ss.sc->host.data(), (size_t)h.sec_len[SEC_SCORES]));
        }
        if (h.n_alts) {      // the list as vox_stream_alternatives reads it: "off" records where it does not reach
            alts.assign((size_t)h.n_alts, AltsState::off());
            std::copy(ss.al->host.begin(), ss.al->host.begin() + std::min(ss.al->host.size(), alts.size()), alts.begin());
            VOXCHK(put(h.sec_off[SEC_ALTS], alts.data(), (size_t)h.sec_len[SEC_ALTS]));
        }
        VOXCHK(put(0, &h, sizeof h));
        HIPCHK(hipStreamSynchronize(s));      // the second: the blob is complete, the staging area may go
        return VOX_OK;
    };
    const int32_t r = body();
    if (r != VOX_OK) (void)hipStreamSynchronize(s);      // (the staging area is freed behind whatever was queued)
    else *nbytes = (size_t)h.total_bytes;
    return r;
}
// every check of a restore, nothing changed: the header (a device blob's is downloaded first), the model, the t_embed, the position limit.  The rate is the
// container's to check (a solo stream refuses another rate, a member takes the blob's).
static int32_t session_restore_check(const SnapSession& ss, const void* blob, size_t nbytes, int32_t mem_kind, vox_snap::SnapHeader* out) {
    using namespace vox_snap;
    ARGCHK(blob, "null argument"); ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    ARGCHK(mem_kind == VOX_MEM_HOST || !(reinterpret_cast<uintptr_t>(blob) & 15), "a device blob must be 16-byte aligned");
    const vox_model_cfg& c = ss.m->cfg;
    SnapHeader h; char msg[256]; unsigned char head[sizeof(SnapHeader)];
    ARGCHK(nbytes >= sizeof head, "snapshot: %zu bytes are shorter than the %zu-byte header", nbytes, sizeof head);
    if (mem_kind == VOX_MEM_DEVICE) HIPCHK(hipMemcpy(head, blob, sizeof head, hipMemcpyDeviceToHost)); else std::memcpy(head, blob, sizeof head);      // a device blob: the header first
    if (!snap_parse(head, nbytes, &h, msg, sizeof msg)) return fail(VOX_ERR_INVALID, "%s", msg);
    uint64_t fp; VOXCHK(model_fingerprint(ss.m, &fp));
    ARGCHK(h.fingerprint == fp, "snapshot: the blob was taken from another model (fingerprint %016llx, this model %016llx)", (unsigned long long)h.fingerprint, (unsigned long long)fp);
    ARGCHK(h.enc_layers == c.enc_layers && h.enc_heads == c.enc_heads && h.enc_head_dim == c.enc_head_dim && h.enc_window == c.enc_window && h.dec_layers == c.dec_layers &&
           h.dec_kv_heads == c.dec_kv_heads && h.dec_head_dim == c.dec_head_dim && h.dec_window == c.dec_window && h.vocab == c.vocab && h.reshape_factor == c.reshape_factor,
           "snapshot: the blob's model geometry is not this model's");
    ARGCHK(h.t_embed_hash == fnv1a(ss.t_embed->data(), ss.t_embed->size() * 4), "snapshot: the blob's session ran with another t_embed than %s", ss.who);
    ARGCHK(h.D >= ss.PC && h.ids_out == h.D - ss.PC, "snapshot: position %d with %d ids handed out (the prefix ends at %d)", h.D, h.ids_out, ss.PC);
    ARGCHK(h.D < ss.max_pos, "snapshot: the blob stands at decoder position %d, %s was created for %d", h.D, ss.who, ss.max_pos);
    ARGCHK(h.We <= ss.cap, "internal: the blob's %d encoder rows exceed the ring of %d", h.We, ss.cap);
    *out = h; return VOX_OK;
}
// the input ring section against the ring the session has at the blob's rate (behind the container's rate step)
static int32_t session_restore_check_ring(const SnapSession& ss, const vox_snap::SnapHeader& h) {
    const FeedState& f = *ss.feed;
    ARGCHK(h.sample_rate == f.sr, "snapshot: the blob's session was fed at %u Hz, %s at %u Hz", h.sample_rate, ss.who, f.sr);
    ARGCHK(h.sec_len[vox_snap::SEC_IN_SAMPLES] == (f.sr != 16000 ? (uint64_t)std::min<int64_t>(h.in_written, f.in_ring_n) * 4 : 0), "snapshot: an input ring section of %llu bytes for a ring of %d samples",
           (unsigned long long)h.sec_len[vox_snap::SEC_IN_SAMPLES], f.in_ring_n);
    return VOX_OK;
}
// the blob's payload into the session's arrays (the container has made room: cache rows or pages, lists), its state block, its host mirror and record lists; ends in
// the call's synchronisation.  `dec` of ss addresses the cache as it is NOW.
static int32_t session_restore_payload(const SnapSession& ss, const vox_snap::SnapHeader& h, const void* blob, int32_t mem_kind) {
    using namespace vox_snap;
    hipStream_t s = ss.ctx->stream; const bool dev = mem_kind == VOX_MEM_DEVICE; FeedState& f = *ss.feed; const char* b = static_cast<const char*>(blob);
    DevBuf stage; const size_t stage_b = dev ? 0 : snap_stage_bytes(h);
    if (stage_b && hipMalloc(&stage.p, stage_b) != hipSuccess) { (void)hipGetLastError(); stage.p = nullptr; return fail(VOX_ERR_HIP, "hipMalloc of the restore's %zu-byte staging area failed", stage_b); }
    std::vector<int32_t> ids((size_t)h.ids_out);
    auto body = [&]() -> int32_t {
        int half = 0; char* wb = const_cast<char*>(b); vox::SnapshotKvParams enc = ss.enc, dec = ss.dec; snap_rows(&enc, &dec, h);
        VOXCHK(snap_move_stack(s, enc, wb + h.sec_off[SEC_ENC_K], wb + h.sec_off[SEC_ENC_V], mem_kind, 1, stage.as<float>(), stage_b, &half));
        VOXCHK(snap_move_stack(s, dec, wb + h.sec_off[SEC_DEC_K], wb + h.sec_off[SEC_DEC_V], mem_kind, 1, stage.as<float>(), stage_b, &half));
        StreamSrc src; src.mem_kind = mem_kind;
        const size_t n16 = (size_t)(h.sec_len[SEC_SAMPLES] / 4), nin = (size_t)(h.sec_len[SEC_IN_SAMPLES] / 4);
        src.p = b + h.sec_off[SEC_SAMPLES]; if (n16) VOXCHK(ring_write_f32(s, ss.samples, STREAM_SAMPLE_RING, h.n_written - (int64_t)n16, src, 0, n16));
        src.p = b + h.sec_off[SEC_IN_SAMPLES]; if (nin) VOXCHK(ring_write_f32(s, f.in_ring, f.in_ring_n, h.in_written - (int64_t)nin, src, 0, nin));
        HIPCHK(hipMemcpyAsync(ss.tokens, b + h.sec_off[SEC_TOKENS], (size_t)h.sec_len[SEC_TOKENS], dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ss.tokens + h.D, &h.token, 4, hipMemcpyHostToDevice, s));      // the header's validated token: the embedding lookup never reads an unchecked index
        std::memset(ss.h_state, 0, sizeof(int) * STRM_WORDS);
        ss.h_state[STRM_POS] = h.D; ss.h_state[STRM_ENC_POS] = h.E; ss.h_state[STRM_FRAME] = 4 * h.E; ss.h_state[STRM_HEAD] = h.E % ss.cap; ss.h_state[STRM_TICKS] = h.D - ss.PC;
        HIPCHK(hipMemcpyAsync(ss.state, ss.h_state, sizeof(int) * STRM_WORDS, hipMemcpyHostToDevice, s));
        // the records: the blob's lists, or the records of ids handed out with the feature off (the ids: the blob's tokens)
        if (h.ids_out) { const char* t = b + h.sec_off[SEC_TOKENS] + (size_t)VOX_PREFIX_TOKENS * 4; if (dev) HIPCHK(hipMemcpyAsync(ids.data(), t, ids.size() * 4, hipMemcpyDeviceToHost, s)); else std::memcpy(ids.data(), t, ids.size() * 4); }
        ss.sc->host.assign((size_t)h.ids_out, vox_token_score{NAN, NAN, -1, 0}); ss.al->host.clear(); ss.al->peeked.clear();
        ss.lv->host.clear(); if (ss.lv->dev) ss.lv->host.assign((size_t)h.ids_out, LevelState::off());      // level records are not carried over: the ids so far have none
        if (h.n_alts) ss.al->host.resize((size_t)h.n_alts);
        if (dev) {
            if (h.n_scores) HIPCHK(hipMemcpyAsync(ss.sc->host.data(), b + h.sec_off[SEC_SCORES], (size_t)h.sec_len[SEC_SCORES], hipMemcpyDeviceToHost, s));
            if (h.n_alts) HIPCHK(hipMemcpyAsync(ss.al->host.data(), b + h.sec_off[SEC_ALTS], (size_t)h.sec_len[SEC_ALTS], hipMemcpyDeviceToHost, s));
        } else {
            if (h.n_scores) std::memcpy(ss.sc->host.data(), b + h.sec_off[SEC_SCORES], (size_t)h.sec_len[SEC_SCORES]);
            if (h.n_alts) std::memcpy(ss.al->host.data(), b + h.sec_off[SEC_ALTS], (size_t)h.sec_len[SEC_ALTS]);
        }
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; !h.n_scores && i < h.ids_out; i++) ss.sc->host[(size_t)i].id = ids[(size_t)i];
        return VOX_OK;
    };
    const int32_t r = body();
    if (r != VOX_OK) { (void)hipStreamSynchronize(s); return r; }
    f.n_pushed = h.n_pushed; f.n_written = h.n_written; f.in_written = h.in_written; f.pos = h.D; f.ids_out = h.ids_out; f.finished = false;
    return VOX_OK;
}

// ---- a solo stream as a SnapSession.  An endless session's cache is addressed as the ring it becomes: below the wrap row % rows is the row
static SnapSession stream_session(vox_stream* st) {
    const vox_model_cfg& c = st->m->cfg; const vox_cache* kc = st->dec;
    SnapSession ss{}; ss.m = st->m; ss.ctx = st->ctx; ss.t_embed = &st->t_embed; ss.feed = &st->feed; ss.sc = &st->sc; ss.al = &st->al; ss.lv = &st->lv; ss.gain = st->gain;
    ss.tokens = st->tokens; ss.samples = st->samples; ss.state = st->state; ss.h_state = st->h_state; ss.cap = st->cap; ss.PC = st->PC; ss.max_pos = st->max_pos; ss.who = "the stream";
    ss.enc.cache_k = st->kring; ss.enc.cache_v = st->vring; ss.enc.layers = c.enc_layers; ss.enc.heads = c.enc_heads; ss.enc.hd = c.enc_head_dim;
    ss.enc.layout = vox::SNAP_RING; ss.enc.cap = st->cap; ss.enc.layer_stride = st->ring_layer; ss.enc.head_stride = (size_t)st->cap * c.enc_head_dim;
    ss.dec.cache_k = kc->k; ss.dec.cache_v = kc->v; ss.dec.layers = c.dec_layers; ss.dec.heads = c.dec_kv_heads; ss.dec.hd = c.dec_head_dim;
    ss.dec.layout = st->endless ? vox::SNAP_RING : vox::SNAP_FLAT; ss.dec.cap = kc->max_seq; ss.dec.layer_stride = kc->layer_stride; ss.dec.head_stride = (size_t)kc->max_seq * c.dec_head_dim;
    return ss;
}
extern "C" int32_t vox_stream_snapshot_size(const vox_stream* st, size_t* nbytes) {
    ARGCHK(st && nbytes, "null argument"); ARGCHK(!st->feed.finished, "the stream is finished: a reset starts its next utterance");
    vox_snap::SnapHeader h; session_snap_header(stream_session(const_cast<vox_stream*>(st)), &h);
    *nbytes = (size_t)h.total_bytes; return VOX_OK;
}
extern "C" int32_t vox_stream_snapshot(vox_stream* st, void* blob, size_t cap, size_t* nbytes, int32_t mem_kind) {
    ARGCHK(st, "null stream"); VOXCHK(ctx_bind(st->ctx));
    return session_snapshot(stream_session(st), blob, cap, nbytes, mem_kind);
}
// the decoder cache rows the doubling rule gives an uninterrupted session that stands at position D (stream_load_initial, stream_tick)
static int stream_dec_rows_at(const vox_stream* st, int D) {
    int rows = std::min(st->dec_limit, ENGINE_MAX_ROWS);
    while (rows < D && rows < st->dec_limit) rows = std::min(st->dec_limit, 2 * rows);
    return rows;
}
extern "C" int32_t vox_stream_restore(vox_stream* st, const void* blob, size_t nbytes, int32_t mem_kind) {
    ARGCHK(st, "null stream"); VOXCHK(ctx_bind(st->ctx));
    vox_model* m = st->m; hipStream_t s = st->ctx->stream;
    // ---- every check, nothing changed
    vox_snap::SnapHeader h; VOXCHK(session_restore_check(stream_session(st), blob, nbytes, mem_kind, &h)); VOXCHK(session_restore_check_ring(stream_session(st), h));
    // ---- allocations (a failure leaves the session what it was): the decoder cache of the rule's size, an endless target's lists
    HIPCHK(hipStreamSynchronize(s));
    const int rows = stream_dec_rows_at(st, h.D);
    vox_cache* fresh = nullptr;
    if (st->dec->max_seq != rows) VOXCHK(cache_alloc(m, rows, &fresh));
    while (st->endless && st->lists_cap < h.D) { const int32_t r = stream_lists_grow(st); if (r != VOX_OK) { (void)hipStreamSynchronize(s); cache_release(fresh); return r; } }
    // ---- from here on the target is the blob's session
    if (fresh) { HIPCHK(hipStreamSynchronize(s)); stream_dec_ungrow(st, &st->peek.old); cache_release(st->dec); st->dec = fresh; }
    st->gain = h.gain;
    int32_t r = VOX_OK;
    if (engine_tab_enqueue(m, st->eng, st->dec) != hipSuccess) r = fail(VOX_ERR_HIP, "uploading the decode engine's layer table failed");      // as stream_load_initial: the first step finds its cache bound
    if (r == VOX_OK && hipMemcpyAsync(&st->d_mem->gain, &st->gain, sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) r = fail(VOX_ERR_HIP, "hipMemcpyAsync failed");
    if (r == VOX_OK) r = session_restore_payload(stream_session(st), h, blob, mem_kind);
    if (r != VOX_OK) { (void)hipStreamSynchronize(s); (void)stream_load_initial(st); return r; }      // a device failure half way: the target is a fresh session, not half of two
    st->dec->len = st->verified_pos = h.D; st->eng_unverified = false;
    st->eng_steps = st->op_steps = st->verified_eng_steps = st->verified_op_steps = 0; st->tap_rows = st->verified_tap_rows = 0; st->ftap_ticks = 0;
    st->bursts = st->burst_ticks = st->single_ticks = 0;
    return VOX_OK;
}

// ---- one launch of the session blob's K / V kernel on host buffers (tests): vox_snapshot_kv_desc's layouts as SnapshotKvParams, ONE launch_snapshot_kv (none when
// lo == hi).  Every argument is checked before the context is bound -- the range against the cache's rows, the ring or the table, every table entry the range touches
// against the pool: nothing the kernel reads or writes lies outside the uploaded buffers.
extern "C" int32_t vox_debug_snapshot_kv(vox_ctx* c, const vox_snapshot_kv_desc* d, float* cache_k, float* cache_v, float* blob, int32_t restore) {
    ARGCHK(c && d && cache_k && cache_v && blob, "null argument");
    ARGCHK(d->head_dim == 64 || d->head_dim == 128, "head_dim %d: the snapshot kernel serves head_dim 64 and 128", d->head_dim);
    ARGCHK(d->layers >= 1 && d->layers <= 64 && d->n_heads >= 1 && d->n_heads <= 64, "bad geometry (%d layers, %d heads)", d->layers, d->n_heads);
    ARGCHK(d->lo >= 0 && d->hi < (1 << 24), "rows %d .. %d outside 0 .. 2^24 - 1", d->lo, d->hi); ARGCHK(d->hi >= d->lo, "hi %d < lo %d", d->hi, d->lo);
    ARGCHK(d->layout >= 0 && d->layout <= 3, "layout %d (0 flat, 1 ring, 2 page table, 3 ring table)", d->layout);
    const int hd = d->head_dim, H = d->n_heads, n = d->hi - d->lo; const bool paged = d->layout >= 2;
    SnapshotKvParams kp{}; kp.layers = d->layers; kp.heads = H; kp.hd = hd; kp.lo = d->lo; kp.hi = d->hi; kp.layout = d->layout;
    size_t cache_f = 0;
    if (!paged) {
        ARGCHK(d->rows >= 1 && d->rows <= 16384, "rows %d out of range (1..16384)", d->rows);
        ARGCHK(!d->page_rows && !d->pool_pages && !d->page_tab_len && !d->page_tab, "a flat or ring call takes no paged field");
        ARGCHK(d->layer_stride >= (int64_t)H * d->rows * hd && d->layer_stride <= ((int64_t)1 << 28) && d->layer_stride % 4 == 0, "layer_stride %lld: a multiple of 4, at least the %lld floats of a layer's rows",
               (long long)d->layer_stride, (long long)H * d->rows * hd);
        if (d->layout == 0) ARGCHK(d->hi <= d->rows, "rows %d .. %d outside the cache's %d rows", d->lo, d->hi, d->rows);
        else ARGCHK(n <= d->rows, "a ring of %d rows is shorter than the %d rows %d .. %d", d->rows, n, d->lo, d->hi);
        kp.cap = d->rows; kp.layer_stride = (size_t)d->layer_stride; kp.head_stride = (size_t)d->rows * hd; cache_f = (size_t)d->layers * kp.layer_stride;
    } else {
        ARGCHK(d->page_rows >= 16 && d->page_rows <= 1024 && !(d->page_rows & (d->page_rows - 1)), "page_rows %d is not a power of two in 16..1024", d->page_rows);
        ARGCHK(!d->rows, "a paged call takes no rows"); ARGCHK(d->page_tab, "null argument (page_tab)");
        ARGCHK(d->pool_pages >= 1 && d->pool_pages <= (1 << 16), "pool_pages %d out of range", d->pool_pages); ARGCHK(d->page_tab_len >= 1 && d->page_tab_len <= 1024, "page_tab_len %d out of range (1..1024)", d->page_tab_len);
        while ((1 << kp.shift) < d->page_rows) kp.shift++;
        kp.page_floats = (size_t)H * d->page_rows * hd; kp.head_stride = (size_t)d->page_rows * hd; kp.layer_stride = kp.page_floats * d->pool_pages; kp.tab_len = d->page_tab_len;
        ARGCHK(d->layer_stride == 0 || (size_t)d->layer_stride == kp.layer_stride, "layer_stride %lld: a paged cache's layers are %zu floats apart", (long long)d->layer_stride, kp.layer_stride);
        if (n > 0) {
            const int pages = ((d->hi - 1) >> kp.shift) - (d->lo >> kp.shift) + 1;
            if (d->layout == 2) ARGCHK(((d->hi - 1) >> kp.shift) < d->page_tab_len, "row %d lies in page %d of a table of %d entries", d->hi - 1, (d->hi - 1) >> kp.shift, d->page_tab_len);
            else ARGCHK(pages <= d->page_tab_len, "rows %d .. %d touch %d pages, the ring table has %d entries", d->lo, d->hi, pages, d->page_tab_len);
            int bad = 0;
            if (!snapshot_kv_pages_ok(d->page_tab, d->layout, kp.shift, d->page_tab_len, d->lo, d->hi, d->pool_pages, &bad))
                return fail(VOX_ERR_INVALID, "table entry %d of the range is %d, outside the pool's %d pages", bad, d->page_tab[d->layout == 3 ? bad % d->page_tab_len : bad], d->pool_pages);
        }
        cache_f = (size_t)d->layers * kp.layer_stride;
    }
    ARGCHK(cache_f <= ((size_t)1 << 28), "a cache of %zu floats is more than this entry uploads", cache_f);
    if (n == 0) return VOX_OK;      // nothing to move: no launch, the arrays stay untouched
    VOXCHK(ctx_bind(c));
    hipStream_t s = c->stream; const size_t plane_f = (size_t)d->layers * H * n * hd;
    DevBuf dk, dv, db, dt;
    HIPCHK(dk.alloc(cache_f * 4)); HIPCHK(dv.alloc(cache_f * 4)); HIPCHK(db.alloc(2 * plane_f * 4)); HIPCHK(dt.alloc(paged ? (size_t)d->page_tab_len * 4 : 4));
    HIPCHK(hipMemcpyAsync(dk.p, cache_k, cache_f * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dv.p, cache_v, cache_f * 4, hipMemcpyHostToDevice, s));
    if (restore) HIPCHK(hipMemcpyAsync(db.p, blob, 2 * plane_f * 4, hipMemcpyHostToDevice, s)); else HIPCHK(hipMemsetAsync(db.p, 0xff, 2 * plane_f * 4, s));      // a word the pack does not write comes back NaN
    if (paged) { HIPCHK(hipMemcpyAsync(dt.p, d->page_tab, (size_t)d->page_tab_len * 4, hipMemcpyHostToDevice, s)); kp.tab = dt.as<int>(); }
    kp.cache_k = dk.as<float>(); kp.cache_v = dv.as<float>(); kp.blob_k = db.as<float>(); kp.blob_v = db.as<float>() + plane_f;
    HIPCHK(launch_snapshot_kv(kp, restore != 0, s));
    HIPCHK(hipMemcpyAsync(cache_k, dk.p, cache_f * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(cache_v, dv.p, cache_f * 4, hipMemcpyDeviceToHost, s));
    if (!restore) HIPCHK(hipMemcpyAsync(blob, db.p, 2 * plane_f * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}

// ------------------------------------------------------------------------------------------------
// Stream group (vox_stream_group; DESIGN.md section 8, "Stream groups"): N <= 16 member sessions on one model, at one t_embed or each at its own, advanced together.  A call knows every
// fed member's due tick count d_i before it launches anything: the members sorted by d_i descending, round r runs ONE tick of the first n_r = #{d_i > r} of them --
// stream_encode_round at 4 n_r rows (the code of a solo stream's tick) and, as the decode half, xf_chain at n_r rows on the group's decoder slab.  One upload (the
// order) per pass, constant launch arguments within a pass except n_r, one synchronisation per call.  No engine runs here: no kept rows, no re-run, no verification.
// A member may be fed at its capture rate, and a call may carry 16-bit PCM: every member's passes are feed_plan / feed_pass on its FeedState, the solo stream's planner;
// the ingest has the member dimension too, one launch per pass (group_stage_pass).
// ONE call path, as a solo stream's: advance, its 16-bit form and peek are group_run; a peek is its mode between the two directions of the ring keep.
// ------------------------------------------------------------------------------------------------
static const int GROUP_MAX = 16, GROUP_DEFAULT_POSITIONS = 2048;
struct GroupMember {
    FeedState feed;                      // the member's host mirror; at a capture rate: its own input ring, a copy of its rate's plan, the rate's matrix (owned by the rate table)
    int rate = -1; uint64_t steps = 0;   // its slot of the group's rate table (-1: 16 kHz); its ticks, each one row of an xf_chain step
    ScoreState sc;                       // its scores (vox_stream_group_set_scores); h_mem[i].scores is sc.dev while they are on
    AltsState al;                        // its alternatives (vox_stream_group_set_alternatives); h_mem[i].alts is al.dev while its k > 0
    LevelState lv;                       // its levels (vox_stream_group_set_levels); h_mem[i].levels is lv.dev while they are on
    int h_state[STRM_WORDS];
    // an endless group's member: its own position-indexed token row of lists_cap + 2 entries (its score and alternatives records have lists_cap + 2 as well), grown
    // by doubling (group_lists_grow).  A bounded group's members share g->tokens and keep 0 / null here
    int* tokens = nullptr; int lists_cap = 0;
};
// one block matrix per rate in use, shared by the members at that rate (built by resample_matrix_build: vox_resample's bits; never the context's matrix, which goes
// when vox_resample serves another rate pair).  refs == 0: a free slot
struct GroupRate { uint32_t sr = 0; ResamplePlan rp; float* At = nullptr; size_t bytes = 0; int refs = 0; };
struct GroupIngest { StreamIngest rs[16]; StreamS16 pcm[16]; };      // a pass's ingest descriptors, one slot per entry of the call: ONE upload
struct vox_stream_group {
    vox_model* m = nullptr; vox_ctx* ctx = nullptr;
    std::vector<float> t_embed; int n = 0; StreamGeom g;
    float *kring = nullptr, *vring = nullptr; size_t ring_layer = 0, ring_member = 0;      // encoder K / V rings: [member][enc_layers][enc_heads][cap][hd]
    float *dec_k = nullptr, *dec_v = nullptr; size_t seq_stride = 0, layer_stride = 0;      // decoder slab: [dec_layers][member][kv_heads][max_pos][hd], the layout xf_chain reads
    float *samples = nullptr, *ws = nullptr; int *tokens = nullptr, *state = nullptr;       // [member][STREAM_SAMPLE_RING], the round's buffers, [member][max_pos + 2], [member][STRM_WORDS]
    StreamMember* d_mem = nullptr; int *d_order = nullptr, *d_pos = nullptr, *d_kv_row = nullptr;      // descriptors [n]; the pass's order, the step's positions and cache slices [16] (one allocation)
    float *qkv = nullptr, *att = nullptr, *logits = nullptr, *ssq = nullptr; uint16_t *xf1 = nullptr, *xf2 = nullptr, *xf3 = nullptr;      // the decode step's rows and XF planes (one 16-row group)
    MelTables mel{}; uint64_t bytes = 0;
    std::vector<StreamMember> h_mem; std::vector<GroupMember> mem;
    std::deque<std::array<int, GROUP_MAX>> orders;      // the orders uploaded by the call in flight (alive until its synchronisation)
    std::vector<GroupRate> rates;
    GroupIngest* d_ingest = nullptr; std::deque<GroupIngest> ingests;      // the pass's ingest descriptors on the device; the ones uploaded by the call in flight, as orders
    int16_t* s16_stage = nullptr;      // host 16-bit feeds: STREAM_SAMPLE_RING samples of device staging per member, allocated at the first one
    int n_scored = 0;                  // members with scores on: a round launches stream_score_kernel only while there is one
    int n_alts = 0;                    // members with alternatives on: the same for stream_alts_kernel
    int n_leveled = 0;                 // members with levels on: the same for stream_level_kernel, in front of the round's mel launch
    KeepArea keep;                     // vox_stream_group_peek: [16 ints: the peeking members, slot by slot][a ring keep area per slot]
    // a paged group (vox_stream_group_create_paged): dec_k / dec_v are the page pool [dec_layers][pool_pages][kv_heads][page_rows][hd] (layer_stride = the floats of a
    // layer's pages), pool the allocator with every member's table mirror, d_tab the device table [n][pool.max_pages], d_kv_page / d_kv_in the step's physical pages and
    // rows inside them [16] (behind d_kv_row, the same allocation).  A slab group: paged == false, nothing of this is set
    bool paged = false; PagePool pool; int* d_tab = nullptr; int *d_kv_page = nullptr, *d_kv_in = nullptr; size_t page_floats = 0;
    // a bf16 paged group (vox_stream_group_create_kv with VOX_KV_BF16; DESIGN.md section 8, "A bf16 K/V pool"): dec_k / dec_v point at uint16_t pools of the same layout
    // -- page_floats, seq_stride and layer_stride then count 16-bit elements.  The allocator, the tables and every refusal are the f32 paged group's
    bool kv_bf16 = false;
    // An ENDLESS paged group (vox_stream_group_create_endless; DESIGN.md section 8, "Endless paged groups"): g.max_pos is 2^24; the pool's tables are rings of pool_pages
    // entries (d_tab [n][pool.tab_len]); every member has its own token row and record lists (GroupMember::tokens, lists_cap), grown by doubling; and the group owns
    // two member-strided device RoPE rings -- decoder [n][GROUP_ROPE_ROWS][cos hd/2 | sin hd/2], encoder [n][R GROUP_ROPE_ROWS][..] -- with their pinned host images,
    // the event behind the last copy out of those images, and the f32 factors of both head dims (rope_inv_fill, computed once).  The rounds of an endless
    // group read the rings at EVERY position: one code path below and above the load-time tables' lengths.
    bool endless = false;
    struct { float *dec = nullptr, *enc = nullptr, *h_dec = nullptr, *h_enc = nullptr; hipEvent_t copied = nullptr; bool pending = false; std::vector<float> inv_d, inv_e; } rope;
    // A BURST group (vox_stream_group_create_burst; DESIGN.md section 8, "Bursts in stream groups"): burst > 1 -- a pass runs every due member's next
    // b_z = min(ticks still due, burst) ticks as ONE encoder pass of 4 sum b_z rows and max b_z decode rounds (group_burst_round); its round buffers hold n burst ticks.
    // d_bdesc: the round's descriptor on the device (a burst group alone), bdescs the ones uploaded by the call in flight, as orders.  burst_rounds / burst_member_ticks:
    // the rounds run with some b_z >= 2 and the member-ticks inside them; plain_rounds: the rounds run as group_round (every group counts them); since create
    int burst = 1; StreamBurstDesc* d_bdesc = nullptr; std::deque<StreamBurstDesc> bdescs; uint64_t burst_rounds = 0, burst_member_ticks = 0, plain_rounds = 0;
    // A group with a DELAY PER MEMBER (vox_stream_group_create_t_embeds; DESIGN.md section 8, "A delay per member"): member_te[i] is member i's t_embed (t_embed above is
    // unread) and ada [n][dec_layers][dec_dim] holds every member's Ada scales -- the model's block as vox_model_set_t_embed(member i's t_embed) fills it, copied device
    // to device when the member is seeded.  The decode round's wo epilogue reads row r's scales through the pass's order; a call never selects the model's t_embed.
    // Every other group: ada == nullptr, member_te empty, and the rounds read the model's one set
    float* ada = nullptr; std::vector<std::vector<float>> member_te;
};
static const std::vector<float>& group_t_embed(const vox_stream_group* g, int i) { return g->ada ? g->member_te[(size_t)i] : g->t_embed; }
static const int GROUP_ROPE_ROWS = 64;         // rows per member of an endless group's decoder RoPE ring: a power of two >= the most ticks of one pass (feed_pass_max_ticks, asserted at create and per pass)
static const int GROUP_LISTS_START = 2048;     // positions an endless group's member lists start with
// entries [q0, q1) of a member's table mirror to the device, on the group's stream (the mirror stays where it is: the tables are sized at create)
// (a ring table: logical pages q0 .. q1 - 1 live at entries q % tab_len -- at most tab_len of them, two copies where the range wraps)
static int32_t group_table_upload(vox_stream_group* g, int member, int64_t q0, int64_t q1) {
    if (q1 <= q0) return VOX_OK;
    const int L = g->pool.tab_len; int* dev = g->d_tab + (size_t)member * L; const int* host = g->pool.mem[(size_t)member].tab.data();
    ARGCHK(q1 - q0 <= L, "internal: member %d: %lld changed table entries, the table has %d", member, (long long)(q1 - q0), L);
    const int e0 = (int)g->pool.slot(q0), cnt = (int)(q1 - q0), k = std::min(cnt, L - e0);
    HIPCHK(hipMemcpyAsync(dev + e0, host + e0, (size_t)k * 4, hipMemcpyHostToDevice, g->ctx->stream));
    if (cnt > k) HIPCHK(hipMemcpyAsync(dev, host, (size_t)(cnt - k) * 4, hipMemcpyHostToDevice, g->ctx->stream));      // the range wrapped (a ring table alone)
    return VOX_OK;
}
// the member leaves its rate: its input ring and its reference to the rate's matrix go (the matrix with its last reference).  The caller has synchronised.
static void group_member_drop_rate(vox_stream_group* g, int i) {
    GroupMember& me = g->mem[i];
    FeedState& f = me.feed;
    if (f.in_ring) (void)hipFree(f.in_ring);
    if (me.rate >= 0) { GroupRate& r = g->rates[(size_t)me.rate]; if (--r.refs == 0) { (void)hipFree(r.At); r = GroupRate{}; } }
    f.sr = 16000; f.rp = ResamplePlan{}; f.At = nullptr; f.in_ring = nullptr; f.in_ring_n = 0; f.in_written = 0; me.rate = -1;
}
// the member's rate from now on.  Everything that can fail happens before anything changes: a refused rate leaves the member as it was.  May synchronise (a new matrix).
static int32_t group_member_set_rate(vox_stream_group* g, int i, uint32_t sr) {
    GroupMember& me = g->mem[i];
    if (sr == me.feed.sr) return VOX_OK;
    ResamplePlan rp; size_t rs_bytes = 0; int ring_n = 0, slot = -1; float *ring = nullptr, *At = nullptr;
    if (sr != 16000) {
        VOXCHK(stream_rate_plan(sr, &rp, &rs_bytes, &ring_n));
        for (size_t k = 0; k < g->rates.size(); k++) if (g->rates[k].refs > 0 && g->rates[k].sr == sr) slot = (int)k;
        if (hipMalloc((void**)&ring, (size_t)ring_n * 4) != hipSuccess) { (void)hipGetLastError(); return fail(VOX_ERR_HIP, "hipMalloc of a member's %d-sample input ring failed", ring_n); }
        if (slot < 0) { const int32_t r = resample_matrix_build(g->ctx, rp, rs_bytes, &At); if (r != VOX_OK) { (void)hipFree(ring); return r; } }
    }
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    group_member_drop_rate(g, i);
    if (sr == 16000) return VOX_OK;
    if (slot < 0) {
        for (size_t k = 0; k < g->rates.size() && slot < 0; k++) if (g->rates[k].refs == 0) slot = (int)k;
        if (slot < 0) { g->rates.emplace_back(); slot = (int)g->rates.size() - 1; }
        GroupRate& r = g->rates[(size_t)slot]; r.sr = sr; r.rp = rp; r.At = At; r.bytes = rs_bytes;
    }
    g->rates[(size_t)slot].refs++;
    FeedState& f = me.feed; f.sr = sr; f.rp = rp; f.At = g->rates[(size_t)slot].At; f.in_ring = ring; f.in_ring_n = ring_n; f.in_written = 0; me.rate = slot;
    return VOX_OK;
}
static int32_t group_upload_members(vox_stream_group* g) {      // after a descriptor changed (gain, tap); synchronises
    HIPCHK(hipMemcpyAsync(g->d_mem, g->h_mem.data(), sizeof(StreamMember) * g->n, hipMemcpyHostToDevice, g->ctx->stream));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    return VOX_OK;
}
// (a group with a delay per member) member i's Ada scales: the model's block for the member's t_embed -- what the seed has just selected, or selects here -- device to device
static int32_t group_member_ada(vox_stream_group* g, int i) {
    if (!g->ada) return VOX_OK;
    const vox_model_cfg& c = g->m->cfg; const size_t n = (size_t)c.dec_layers * c.dec_dim;
    VOXCHK(vox_model_set_t_embed(g->m, g->member_te[(size_t)i].data()));      // (equal bits: returns at once)
    HIPCHK(hipMemcpyAsync(g->ada + (size_t)i * n, g->m->ada_mul, n * 4, hipMemcpyDeviceToDevice, g->ctx->stream));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    return VOX_OK;
}
static int32_t group_member_seed(vox_stream_group* g, int i) {
    if (g->paged) {      // every page the member holds goes back, the prefix rows go into fresh ones (the top of the stack: the pages just returned)
        const vox_model_cfg& c = g->m->cfg; GroupMember& me = g->mem[i]; int64_t q0, q1, t0, t1;
        ARGCHK(g->pool.held(i) + g->pool.n_free() >= (g->g.PC + g->pool.page_rows - 1) / g->pool.page_rows, "member %d: the pool has no pages for the seed", i);
        g->pool.release_all(i, &q0, &q1);
        if (!g->pool.take(i, g->g.PC, &t0, &t1)) return fail(VOX_ERR_INVALID, "internal: member %d: no pool pages for the seed", i);
        VOXCHK(stream_seed(g->m, group_t_embed(g, i).data(), g->g.RC, g->g.PC, g->g.cap, g->h_mem[i].kring, g->h_mem[i].vring, nullptr, g->h_mem[i].tokens, g->h_mem[i].state, me.h_state,
                           [&]() -> int32_t {
                               if (g->endless) { VOXCHK(group_table_upload(g, i, q0, q1)); VOXCHK(group_table_upload(g, i, t0, t1)); }      // (the returned pages may lie anywhere in the ring; the seed's are entries 0 ..)
                               else VOXCHK(group_table_upload(g, i, 0, std::max(q1, t1)));
                               HIPCHK(launch_stream_pages_seed(g->m->pfx.dec_k, g->m->pfx.dec_v, c.dec_layers, c.dec_kv_heads, g->g.PC, c.dec_head_dim, g->d_tab + (size_t)i * g->pool.tab_len,
                                                               g->pool.shift, g->layer_stride, g->dec_k, g->dec_v, g->ctx->stream, g->kv_bf16));
                               return VOX_OK; }));
        me.feed.restart(g->g.PC); me.steps = 0; me.sc.host.clear(); me.al.restart(); me.lv.restart();
        return group_member_ada(g, i);
    }
    vox_cache view; view.m = g->m; view.ctx = g->ctx; view.k = g->dec_k + (size_t)i * g->seq_stride; view.v = g->dec_v + (size_t)i * g->seq_stride; view.max_seq = g->g.max_pos;
    view.layer_stride = g->layer_stride;      // the member's slice of the slab, seen as a cache whose layers lie layer_stride apart
    GroupMember& me = g->mem[i];
    VOXCHK(stream_seed(g->m, group_t_embed(g, i).data(), g->g.RC, g->g.PC, g->g.cap, g->h_mem[i].kring, g->h_mem[i].vring, &view, g->h_mem[i].tokens, g->h_mem[i].state, me.h_state,
                       []() -> int32_t { return VOX_OK; }));
    me.feed.restart(g->g.PC); me.steps = 0; me.sc.host.clear(); me.al.restart(); me.lv.restart();
    return group_member_ada(g, i);
}
static void group_release(vox_stream_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device); (void)hipStreamSynchronize(g->ctx->stream);      // never dereferences g->m (as stream_release)
    for (StreamMember& me : g->h_mem) if (me.tap) (void)hipFree(me.tap);
    for (GroupMember& me : g->mem) { if (me.sc.dev) (void)hipFree(me.sc.dev); if (me.al.dev) (void)hipFree(me.al.dev); if (me.lv.dev) (void)hipFree(me.lv.dev); if (me.tokens) (void)hipFree(me.tokens); }
    for (void* p : {(void*)g->rope.dec, (void*)g->rope.enc}) if (p) (void)hipFree(p);
    if (g->rope.h_dec) (void)hipHostFree(g->rope.h_dec); if (g->rope.h_enc) (void)hipHostFree(g->rope.h_enc);
    if (g->rope.copied) (void)hipEventDestroy(g->rope.copied);
    for (size_t i = 0; i < g->mem.size(); i++) group_member_drop_rate(g, (int)i);
    for (void* p : {(void*)g->keep.p, (void*)g->d_ingest, (void*)g->s16_stage, (void*)g->kring, (void*)g->vring, (void*)g->dec_k, (void*)g->dec_v, (void*)g->samples, (void*)g->ws, (void*)g->tokens, (void*)g->state, (void*)g->d_mem, (void*)g->d_order,
                    (void*)g->qkv, (void*)g->att, (void*)g->logits, (void*)g->ssq, (void*)g->xf1, (void*)g->xf2, (void*)g->xf3, (void*)g->d_tab, (void*)g->d_bdesc, (void*)g->ada}) if (p) (void)hipFree(p);
    delete g;
}
// page_rows < 0: a slab group (pool_pages unread); else a paged one (0: the default page / the default pool)
// endless (a paged group alone): max_positions is unread, the limit is the session limit 2^24
// per_member: t_embed holds [n_members][dec_dim], one delay per member (vox_stream_group_create_t_embeds); else one [dec_dim] vector for all
static int32_t group_create(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                            int32_t max_positions, int32_t page_rows, int32_t pool_pages, vox_stream_group** out, bool endless = false, bool kv_bf16 = false, int burst = 1,
                            bool per_member = false) {
    ARGCHK(burst >= 1 && burst <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst, VOX_STREAM_BURST_MAX);
    ARGCHK(n_members >= 1 && n_members <= GROUP_MAX, "n_members %d out of range (1..%d)", n_members, GROUP_MAX); ARGCHK(m && t_embed && out, "null argument");
    for (int i = 0; gains && i < n_members; i++) ARGCHK(std::isfinite(gains[i]), "gain of member %d is not finite", i);
    for (int i = 0; rates && i < n_members; i++) {      // every rate is checked before anything is allocated
        ARGCHK(rates[i] > 0, "member %d: bad sample rate 0", i);
        if (rates[i] != 16000) { ResamplePlan rp; size_t b; int rn; VOXCHK(stream_rate_plan(rates[i], &rp, &b, &rn)); }
    }
    VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    const bool paged = page_rows >= 0;
    ARGCHK(!endless || paged, "internal: an endless group is a paged one"); ARGCHK(!kv_bf16 || paged, "internal: a bf16 K/V pool belongs to a paged group");
    StreamGeom sg; VOXCHK(stream_geometry(m, enc_capacity_rows, endless ? 0 : max_positions, paged ? INT32_MAX : GROUP_DEFAULT_POSITIONS, &sg, burst));      // (paged, 0: the session limit)
    if (endless) {
        ARGCHK(c.dec_window >= 0, "an endless group needs a sliding decoder window");
        // a pass runs at most the ticks whose samples the 65 536-sample ring holds: each of them has a row of its own in the member's RoPE rings
        ARGCHK(feed_pass_max_ticks(c.reshape_factor) <= GROUP_ROPE_ROWS, "internal: a pass may run %d ticks, the RoPE rings hold %d rows per member", feed_pass_max_ticks(c.reshape_factor), GROUP_ROPE_ROWS);
        // a burst round's attention reads the R b RoPE rows of a member's next b ticks in one launch: the pass's refill has written them, and they are distinct ring rows
        ARGCHK(GROUP_ROPE_ROWS * c.reshape_factor >= 4 * burst, "internal: a burst of %d ticks reads %d encoder RoPE rows, a member's ring holds %d", burst, 4 * burst, GROUP_ROPE_ROWS * c.reshape_factor);
        sg.max_pos = STREAM_POS_LIMIT;
    }
    if (paged) {
        if (page_rows == 0) page_rows = PAGE_ROWS_DEFAULT;
        ARGCHK(page_rows_ok(page_rows), "page_rows %d is not a power of two in %d..%d", page_rows, PAGE_ROWS_MIN, PAGE_ROWS_MAX);
        const int seed = (sg.PC + page_rows - 1) / page_rows, most = (sg.max_pos + page_rows - 1) / page_rows;
        ARGCHK(pool_pages >= 0, "pool_pages %d is negative", pool_pages);
        if (pool_pages == 0) pool_pages = n_members * std::min(most, std::max(seed, (GROUP_DEFAULT_POSITIONS + page_rows - 1) / page_rows));      // the default slab's memory
        ARGCHK(pool_pages >= n_members * seed, "a pool of %d pages cannot hold the seeds of %d members (%d pages each)", pool_pages, n_members, seed);
        ARGCHK(pool_pages <= n_members * most, "a pool of %d pages is more than %d members of %d positions can hold (%d)", pool_pages, n_members, sg.max_pos, n_members * most);
    }
    if (!batch_xf_ok(m)) return fail(VOX_ERR_UNSUPPORTED, "a stream group's decode step runs on the tile-ordered Q4 weights, which this model does not have");
    if (!paged && attn_decode_takes_gqa(c.dec_head_dim, c.dec_heads, c.dec_kv_heads)) {      // the slab's step is xf_chain with prefer_gqa: its attention keeps 16 bytes of LDS per slab row
        int most = 0; HIPCHK(attn_decode_gqa_max_seq(&most));
        ARGCHK(sg.max_pos <= most, "max_positions %d: a slab group of this model serves at most %d positions (its GQA decode attention keeps 16 bytes of LDS per position); "
                                   "a paged group (vox_stream_group_create_paged) has no such limit", sg.max_pos, most);
    }
    VOXCHK(enc_stream_rope_ensure(m));
    vox_stream_group* g = new vox_stream_group(); g->m = m; g->ctx = cx; g->n = n_members;
    if (per_member) for (int i = 0; i < n_members; i++) g->member_te.emplace_back(t_embed + (size_t)i * c.dec_dim, t_embed + (size_t)(i + 1) * c.dec_dim);
    else g->t_embed.assign(t_embed, t_embed + c.dec_dim);
    g->g = sg; g->endless = endless; g->kv_bf16 = kv_bf16; g->burst = burst;
    const size_t N = (size_t)n_members; const int D = c.dec_dim, QD = c.dec_heads * c.dec_head_dim, W = QD + 2 * c.dec_kv_heads * c.dec_head_dim, maxp = sg.max_pos;
    g->ring_layer = (size_t)c.enc_heads * sg.cap * c.enc_head_dim; g->ring_member = (size_t)c.enc_layers * g->ring_layer;
    g->seq_stride = (size_t)c.dec_kv_heads * maxp * c.dec_head_dim; g->layer_stride = N * g->seq_stride;
    if (paged) {
        g->paged = true;
        if (endless) g->pool.init_ring(n_members, page_rows, c.dec_window, pool_pages, STREAM_POS_LIMIT); else g->pool.init(n_members, page_rows, c.dec_window, pool_pages, maxp);
        g->page_floats = (size_t)c.dec_kv_heads * page_rows * c.dec_head_dim; g->seq_stride = g->page_floats; g->layer_stride = (size_t)pool_pages * g->page_floats;
    }
    const size_t ws_b = stream_ws_carve(m, n_members, nullptr, nullptr, burst) * 4, slab_b = (size_t)c.dec_layers * g->layer_stride * (kv_bf16 ? 2 : 4);
    hipError_t e = hipSuccess;
    auto A = [&](void** q, size_t nb, bool zero) { if (e == hipSuccess) { e = hipMalloc(q, nb); if (e == hipSuccess) { g->bytes += nb; if (zero) e = hipMemsetAsync(*q, 0, nb, s); } } };
    A((void**)&g->kring, N * g->ring_member * 4, false); A((void**)&g->vring, N * g->ring_member * 4, false); A((void**)&g->dec_k, slab_b, true); A((void**)&g->dec_v, slab_b, true);
    A((void**)&g->samples, N * STREAM_SAMPLE_RING * 4, true); A((void**)&g->ws, ws_b, true); if (!endless) A((void**)&g->tokens, N * (maxp + 2) * 4, true); A((void**)&g->state, N * sizeof(int) * STRM_WORDS, true);
    A((void**)&g->d_mem, N * sizeof(StreamMember), true); A((void**)&g->d_order, 5 * GROUP_MAX * 4, true);
    if (paged) A((void**)&g->d_tab, N * (size_t)g->pool.tab_len * 4, false); A((void**)&g->d_ingest, sizeof(GroupIngest), true);
    if (burst > 1) A((void**)&g->d_bdesc, sizeof(StreamBurstDesc), true);
    if (per_member) A((void**)&g->ada, N * c.dec_layers * c.dec_dim * 4, true);
    A((void**)&g->qkv, (size_t)GROUP_MAX * W * 4, true); A((void**)&g->att, (size_t)GROUP_MAX * QD * 4, true); A((void**)&g->logits, (size_t)GROUP_MAX * c.vocab * 4, true);
    A((void**)&g->ssq, (size_t)q4_skinny_resid_xf_parts(D) * 16 * 4, true); A((void**)&g->xf1, xf_bytes(D), true); A((void**)&g->xf2, xf_bytes(QD), true); A((void**)&g->xf3, xf_bytes(c.dec_ffn), true);
    g->h_mem.resize(N); g->mem.resize(N);
    if (endless) {      // the members' own token rows (counted per member: vox_stream_group_info), the RoPE rings and their pinned host images (group_rope_refill)
        const size_t db = N * GROUP_ROPE_ROWS * c.dec_head_dim * 4, eb = N * GROUP_ROPE_ROWS * c.reshape_factor * c.enc_head_dim * 4;
        for (size_t i = 0; i < N && e == hipSuccess; i++) {
            g->mem[i].lists_cap = GROUP_LISTS_START; e = hipMalloc((void**)&g->mem[i].tokens, (size_t)(GROUP_LISTS_START + 2) * 4);
            if (e == hipSuccess) e = hipMemsetAsync(g->mem[i].tokens, 0, (size_t)(GROUP_LISTS_START + 2) * 4, s);
        }
        A((void**)&g->rope.dec, db, true); A((void**)&g->rope.enc, eb, true);
        if (e == hipSuccess) e = hipHostMalloc((void**)&g->rope.h_dec, db, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&g->rope.h_enc, eb, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->rope.copied, hipEventDisableTiming);
        g->rope.inv_d.resize((size_t)c.dec_head_dim / 2); g->rope.inv_e.resize((size_t)c.enc_head_dim / 2);
        rope_inv_fill(c.dec_head_dim, c.rope_theta, g->rope.inv_d.data()); rope_inv_fill(c.enc_head_dim, c.rope_theta, g->rope.inv_e.data());
    }
    if (e != hipSuccess) { (void)hipGetLastError(); group_release(g); return fail(VOX_ERR_HIP, "allocating the stream group's device state failed: %s", hipGetErrorString(e)); }
    g->d_pos = g->d_order + GROUP_MAX; g->d_kv_row = g->d_pos + GROUP_MAX; g->d_kv_page = g->d_kv_row + GROUP_MAX; g->d_kv_in = g->d_kv_page + GROUP_MAX;
    if (paged) e = hipMemsetAsync(g->d_tab, 0xff, N * (size_t)g->pool.tab_len * 4, s);      // every entry -1
    if (e != hipSuccess) { (void)hipGetLastError(); group_release(g); return fail(VOX_ERR_HIP, "initialising the stream group's page table failed: %s", hipGetErrorString(e)); }
    for (size_t i = 0; i < N; i++) {
        StreamMember& me = g->h_mem[i]; me = StreamMember{};
        me.samples = g->samples + i * STREAM_SAMPLE_RING; me.gain = gains ? gains[i] : 1.0f; me.state = g->state + i * STRM_WORDS;
        me.kring = g->kring + i * g->ring_member; me.vring = g->vring + i * g->ring_member; me.tokens = endless ? g->mem[i].tokens : g->tokens + i * (size_t)(maxp + 2);
    }
    int32_t r = ctx_mel_tables(cx, &g->mel);
    if (r == VOX_OK) r = group_upload_members(g);
    for (int i = 0; i < n_members && r == VOX_OK; i++) r = group_member_seed(g, i);
    for (int i = 0; rates && i < n_members && r == VOX_OK; i++) r = group_member_set_rate(g, i, rates[i]);
    if (r != VOX_OK) { group_release(g); return r; }
    *out = g; return VOX_OK;
}
extern "C" int32_t vox_stream_group_create_rates(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                                 int32_t max_positions, vox_stream_group** out) {
    return group_create(m, t_embed, n_members, gains, rates, enc_capacity_rows, max_positions, -1, 0, out);
}
extern "C" int32_t vox_stream_group_create_paged(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                                 int32_t max_positions, int32_t page_rows, int32_t pool_pages, vox_stream_group** out) {
    ARGCHK(page_rows >= 0, "page_rows %d is negative", page_rows);
    return group_create(m, t_embed, n_members, gains, rates, enc_capacity_rows, max_positions, page_rows, pool_pages, out);
}
extern "C" int32_t vox_stream_group_create_endless(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                                   int32_t page_rows, int32_t pool_pages, vox_stream_group** out) {
    ARGCHK(page_rows >= 0, "page_rows %d is negative", page_rows);
    return group_create(m, t_embed, n_members, gains, rates, enc_capacity_rows, 0, page_rows, pool_pages, out, true);
}
extern "C" int32_t vox_stream_group_create_kv(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                              int32_t max_positions, int32_t page_rows, int32_t pool_pages, int32_t endless, int32_t kv_dtype, vox_stream_group** out) {
    ARGCHK(kv_dtype == VOX_KV_F32 || kv_dtype == VOX_KV_BF16, "kv_dtype %d is neither VOX_KV_F32 (0) nor VOX_KV_BF16 (1)", kv_dtype);
    ARGCHK(endless == 0 || endless == 1, "endless %d is neither 0 nor 1", endless);
    ARGCHK(!endless || max_positions == 0, "an endless group takes no max_positions (%d): its members go on to the session limit", max_positions);
    ARGCHK(page_rows >= 0, "page_rows %d is negative", page_rows);
    return group_create(m, t_embed, n_members, gains, rates, enc_capacity_rows, endless ? 0 : max_positions, page_rows, pool_pages, out, endless != 0, kv_dtype == VOX_KV_BF16);
}
extern "C" int32_t vox_stream_group_create_burst(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                                 int32_t max_positions, int32_t paged, int32_t page_rows, int32_t pool_pages, int32_t endless, int32_t kv_dtype, int32_t burst_ticks,
                                                 vox_stream_group** out) {
    ARGCHK(m && t_embed && out, "null argument");
    ARGCHK(burst_ticks >= 1 && burst_ticks <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst_ticks, VOX_STREAM_BURST_MAX);
    ARGCHK(paged == 0 || paged == 1, "paged %d is neither 0 nor 1", paged); ARGCHK(endless == 0 || endless == 1, "endless %d is neither 0 nor 1", endless);
    ARGCHK(kv_dtype == VOX_KV_F32 || kv_dtype == VOX_KV_BF16, "kv_dtype %d is neither VOX_KV_F32 (0) nor VOX_KV_BF16 (1)", kv_dtype);
    ARGCHK(paged || (!page_rows && !pool_pages && !endless && kv_dtype == VOX_KV_F32), "a slab group (paged 0) takes no page_rows, pool_pages, endless or bf16 pool");
    ARGCHK(page_rows >= 0, "page_rows %d is negative", page_rows);
    ARGCHK(!endless || max_positions == 0, "an endless group takes no max_positions (%d): its members go on to the session limit", max_positions);
    return group_create(m, t_embed, n_members, gains, rates, enc_capacity_rows, endless ? 0 : max_positions, paged ? page_rows : -1, pool_pages, out, endless != 0, kv_dtype == VOX_KV_BF16, burst_ticks);
}
// the full-argument creator with a t_embed per member: every kind of group (burst_ticks 1: a plain one)
extern "C" int32_t vox_stream_group_create_t_embeds(vox_model* m, const float* t_embeds, int32_t n_members, const float* gains, const uint32_t* rates, int32_t enc_capacity_rows,
                                                    int32_t max_positions, int32_t paged, int32_t page_rows, int32_t pool_pages, int32_t endless, int32_t kv_dtype, int32_t burst_ticks,
                                                    vox_stream_group** out) {
    ARGCHK(m && t_embeds && out, "null argument");
    ARGCHK(n_members >= 1 && n_members <= GROUP_MAX, "n_members %d out of range (1..%d)", n_members, GROUP_MAX);      // (before t_embeds is read as n_members rows)
    ARGCHK(burst_ticks >= 1 && burst_ticks <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst_ticks, VOX_STREAM_BURST_MAX);
    ARGCHK(paged == 0 || paged == 1, "paged %d is neither 0 nor 1", paged); ARGCHK(endless == 0 || endless == 1, "endless %d is neither 0 nor 1", endless);
    ARGCHK(kv_dtype == VOX_KV_F32 || kv_dtype == VOX_KV_BF16, "kv_dtype %d is neither VOX_KV_F32 (0) nor VOX_KV_BF16 (1)", kv_dtype);
    ARGCHK(paged || (!page_rows && !pool_pages && !endless && kv_dtype == VOX_KV_F32), "a slab group (paged 0) takes no page_rows, pool_pages, endless or bf16 pool");
    ARGCHK(page_rows >= 0, "page_rows %d is negative", page_rows);
    ARGCHK(!endless || max_positions == 0, "an endless group takes no max_positions (%d): its members go on to the session limit", max_positions);
    return group_create(m, t_embeds, n_members, gains, rates, enc_capacity_rows, endless ? 0 : max_positions, paged ? page_rows : -1, pool_pages, out, endless != 0, kv_dtype == VOX_KV_BF16, burst_ticks, true);
}
extern "C" int32_t vox_stream_group_t_embed(const vox_stream_group* g, int32_t member, float* out, int32_t cap) {
    ARGCHK(g && out, "null argument"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    const std::vector<float>& te = group_t_embed(g, member);
    ARGCHK(cap >= (int32_t)te.size(), "cap %d: a t_embed of this model has %d values", cap, (int)te.size());
    std::memcpy(out, te.data(), te.size() * 4);
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_burst_info(const vox_stream_group* g, int64_t out[4]) {
    ARGCHK(g && out, "null argument");
    out[0] = g->burst; out[1] = (int64_t)g->burst_rounds; out[2] = (int64_t)g->burst_member_ticks; out[3] = (int64_t)g->plain_rounds;
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_pool(const vox_stream_group* g, int64_t out[4], int32_t* held_or_null) {
    ARGCHK(g && out, "null argument");
    if (!g->paged) return fail(VOX_ERR_UNSUPPORTED, "a slab group has no page pool (vox_stream_group_create_paged makes a paged one)");
    out[0] = g->pool.page_rows; out[1] = g->pool.pool_pages; out[2] = g->pool.n_free(); out[3] = g->pool.peak;
    for (int i = 0; held_or_null && i < g->n; i++) held_or_null[i] = g->pool.held(i);
    return VOX_OK;
}
extern "C" int32_t vox_debug_stream_group_pages(const vox_stream_group* g, int32_t member, int32_t* out, int32_t cap, int32_t* n) {
    ARGCHK(g && n && (out || cap == 0) && cap >= 0, "bad argument"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    if (!g->paged) return fail(VOX_ERR_UNSUPPORTED, "a slab group has no pages");
    const PagePool::Member& me = g->pool.mem[(size_t)member];
    for (int64_t q = me.first; q < me.end && q - me.first < cap; q++) out[q - me.first] = g->pool.at(member, q);
    *n = (int32_t)(me.end - me.first);
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_create(vox_model* m, const float* t_embed, int32_t n_members, const float* gains, int32_t enc_capacity_rows, int32_t max_positions,
                                           vox_stream_group** out) {
    return vox_stream_group_create_rates(m, t_embed, n_members, gains, nullptr, enc_capacity_rows, max_positions, out);
}
extern "C" int32_t vox_stream_group_free(vox_stream_group* g) { group_release(g); return VOX_OK; }
// sample_rate 0: the member keeps its rate (vox_stream_group_reset)
static int32_t group_reset(vox_stream_group* g, int32_t member, float gain, uint32_t sample_rate) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1); ARGCHK(std::isfinite(gain), "gain is not finite");
    VOXCHK(ctx_bind(g->ctx));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    if (sample_rate) VOXCHK(group_member_set_rate(g, member, sample_rate));      // refused: the member, its rate and its state are as they were
    g->h_mem[member].gain = gain;
    VOXCHK(group_upload_members(g));
    return group_member_seed(g, member);      // (the state block restarts the tap's row count as well)
}
extern "C" int32_t vox_stream_group_reset(vox_stream_group* g, int32_t member, float gain) { return group_reset(g, member, gain, 0); }
extern "C" int32_t vox_stream_group_reset_rate(vox_stream_group* g, int32_t member, float gain, uint32_t sample_rate) {
    ARGCHK(g, "null group"); ARGCHK(sample_rate > 0, "bad sample rate 0");
    return group_reset(g, member, gain, sample_rate);
}
// the member's next utterance at another delay (a group with a delay per member alone).  Everything that can refuse comes first: the member, its delay and its state
// are then as they were.  Behind the checks: the host copy, then the ordinary reset, whose seed starts from the prefix state of the new t_embed and copies its scales
extern "C" int32_t vox_stream_group_reset_t_embed(vox_stream_group* g, int32_t member, float gain, uint32_t sample_rate, const float* t_embed) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1); ARGCHK(std::isfinite(gain), "gain is not finite");
    ARGCHK(t_embed, "member %d: null t_embed", member);
    if (!g->ada) return fail(VOX_ERR_UNSUPPORTED, "member %d: this group runs every member at one t_embed (vox_stream_group_create_t_embeds makes one with a delay per member)", member);
    if (sample_rate && sample_rate != 16000) { ResamplePlan rp; size_t b; int rn; VOXCHK(stream_rate_plan(sample_rate, &rp, &b, &rn)); }
    VOXCHK(ctx_bind(g->ctx));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    if (sample_rate) VOXCHK(group_member_set_rate(g, member, sample_rate));      // refused: nothing has changed
    g->member_te[(size_t)member].assign(t_embed, t_embed + g->m->cfg.dec_dim);
    return group_reset(g, member, gain, 0);
}
extern "C" int32_t vox_stream_group_info(const vox_stream_group* g, int32_t member, int64_t out[8]) {
    ARGCHK(g && out, "null argument"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    const GroupMember& me = g->mem[member]; const int R = g->m->cfg.reshape_factor;
    const uint64_t tap_b = g->h_mem[member].tap ? (uint64_t)g->h_mem[member].tap_max * g->m->cfg.vocab * 4 : 0;
    const uint64_t rate_b = me.rate >= 0 ? (uint64_t)me.feed.in_ring_n * 4 + g->rates[(size_t)me.rate].bytes / (uint64_t)g->rates[(size_t)me.rate].refs : 0;
    feed_info(me.feed, R, g->g.cap, out);
    const uint64_t tok_b = me.tokens ? (uint64_t)(me.lists_cap + 2) * 4 : 0;      // (an endless group's member: its own token row, as it is)
    out[5] = (int64_t)(g->bytes / (uint64_t)g->n + tap_b + rate_b + tok_b + me.sc.bytes() + me.al.bytes() + me.lv.bytes());      // the member's share of the group's device state; its own input ring, its share of its rate's matrix, its score, alternatives and level records
    out[6] = 0; out[7] = (int64_t)me.steps;                      // no engine step; the member's ticks, each one row of an xf_chain step
    return VOX_OK;
}

static StreamRound group_stream_round(const vox_stream_group* g, int n_r) {
    StreamRound r{g->d_mem, g->d_order, n_r, g->g.cap, g->ring_layer, g->mel, g->g.left}; r.levels = g->n_leveled > 0;      // (slots of members with levels off return at once)
    if (g->endless) { r.rope = g->rope.enc; r.rope_stride = GROUP_ROPE_ROWS * g->m->cfg.reshape_factor; r.rope_mask = r.rope_stride - 1; }      // every position: the member's ring row (group_rope_refill)
    return r;
}
// the decode half of a round for the first n_r members of the pass's order: the embed (row r's adapter row is w.arow[r]; bd: decode round t of a burst round, the row is
// w.arow[bd->tick0[r] + t]), xf_chain on the group's decoder cache, the advance, the records
static int32_t group_decode_round(vox_stream_group* g, const StreamWs& w, int n_r, const StreamBurstDesc* bd = nullptr, int t = 0) {
    vox_model* m = g->m; const vox_model_cfg& c = m->cfg; hipStream_t s = g->ctx->stream; const int R = c.reshape_factor;
    XfBufs xb{}; xb.h = w.h; xb.qkv = g->qkv; xb.att = g->att; xb.logits = g->logits; xb.ssq = g->ssq; xb.xf1 = g->xf1; xb.xf2 = g->xf2; xb.xf3 = g->xf3;
    xb.k = g->dec_k; xb.v = g->dec_v; xb.layer_stride = g->layer_stride; xb.seq_stride = g->seq_stride; xb.max_seq = g->endless ? 0 : g->g.max_pos; xb.pos = g->d_pos; xb.kv_row = g->d_kv_row;      // (a paged step never reads max_seq)
    StreamPages pg{g->d_tab, g->pool.tab_len, g->pool.shift, g->d_kv_page, g->d_kv_in, g->endless ? g->pool.tab_len : 0};
    if (g->endless) { xb.page_tab_len = g->pool.tab_len; xb.rope_ring = g->rope.dec; xb.rope_mask = GROUP_ROPE_ROWS - 1; }
    xb.kv_bf16 = g->kv_bf16 ? 1 : 0;
    if (g->ada) { xb.ada_rows = g->ada; xb.ada_order = g->d_order; xb.ada_stride = (long)c.dec_layers * c.dec_dim; }      // row r is member order[r]: a prefix of the pass's order in a burst's late rounds too
    if (g->paged) {
        xb.page_tab = g->d_tab; xb.page_tab_stride = g->pool.tab_len; xb.page_shift = g->pool.shift; xb.page_floats = (long)g->page_floats; xb.kv_page = g->d_kv_page; xb.kv_in = g->d_kv_in;
        xb.score_rows = c.dec_window >= 0 ? std::min(g->g.max_pos, c.dec_window + 1) : g->g.max_pos;
    }
    if (bd) HIPCHK(launch_stream_group_embed_burst(m->tok.w, g->d_mem, g->d_order, n_r, w.arow, bd, t, c.dec_dim, w.h, g->xf1, m->dec[0].attn_norm, g->ssq, g->d_pos, g->d_kv_row, s, g->paged ? &pg : nullptr));
    else HIPCHK(launch_stream_group_embed(m->tok.w, g->d_mem, g->d_order, n_r, w.arow, c.dec_dim, w.h, g->xf1, m->dec[0].attn_norm, g->ssq, g->d_pos, g->d_kv_row, s, g->paged ? &pg : nullptr));
    VOXCHK(xf_chain(m, xb, 0, n_r, 0, 0, true, 0, s));
    HIPCHK(launch_stream_group_advance(g->logits, c.vocab, g->d_mem, g->d_order, n_r, R, 4 * R, g->g.cap, s));
    if (g->n_scored > 0) HIPCHK(launch_stream_score(g->logits, c.vocab, g->d_mem, g->d_order, n_r, VOX_PREFIX_TOKENS, s));      // slots of unscored members return at once
    if (g->n_alts > 0) HIPCHK(launch_stream_alts(g->logits, c.vocab, g->d_mem, g->d_order, n_r, VOX_PREFIX_TOKENS, s));      // (the same)
    return VOX_OK;
}
// one round: a tick of the first n_r members of the pass's order
static int32_t group_round(vox_stream_group* g, const StreamWs& w, int n_r) {
    VOXCHK(stream_encode_round(g->m, w, group_stream_round(g, n_r), nullptr, nullptr));
    g->plain_rounds++;
    return group_decode_round(g, w, n_r);
}
// one BURST round of a burst group: the first n_r members of the pass's order run b[z] ticks each (descending, b[0] >= 2) -- ONE encoder pass of R sum b rows
// (stream_encode_round's ragged form; the round's descriptor goes up once and stays alive until the call's synchronisation), then the b[0] decode rounds one by one:
// decode round t serves the members with b[z] > t, a prefix of the order.  The encoder reads every member's state block as its first tick of the round finds it; the
// b[z] advance launches leave it as b[z] ticks would.
static int32_t group_burst_round(vox_stream_group* g, const StreamWs& w, int n_r, const int* b) {
    ARGCHK(g->burst > 1 && g->d_bdesc && n_r >= 1 && n_r <= GROUP_MAX && b[0] >= 2 && b[0] <= g->burst, "internal: a burst round of %d members, %d ticks at most (burst_ticks %d)", n_r, b[0], g->burst);
    g->bdescs.emplace_back(); StreamBurstDesc& d = g->bdescs.back(); std::memset(&d, 0, sizeof d);
    int ticks = 0;
    for (int z = 0; z < n_r; z++) { ARGCHK(b[z] >= 1 && (z == 0 || b[z] <= b[z - 1]), "internal: slot %d of a burst round runs %d ticks", z, b[z]); d.tick0[z] = ticks; d.b[z] = b[z]; ticks += b[z]; }
    HIPCHK(hipMemcpyAsync(g->d_bdesc, &d, sizeof d, hipMemcpyHostToDevice, g->ctx->stream));      // the round's one descriptor upload
    const StreamRagged rg{g->d_bdesc, &d, ticks};
    VOXCHK(stream_encode_round(g->m, w, group_stream_round(g, n_r), nullptr, nullptr, b[0], 1, &rg));
    int n_t = n_r;
    for (int t = 0; t < b[0]; t++) {
        while (b[n_t - 1] <= t) n_t--;
        VOXCHK(group_decode_round(g, w, n_t, g->d_bdesc, t));
    }
    g->burst_rounds++; g->burst_member_ticks += (uint64_t)ticks;
    return VOX_OK;
}
// A group's call -- advance, its 16-bit form, peek -- is group_run, in four units: group_plan_entries (every check, nothing changed), then per pass group_stage_pass
// (feed_pass for every entry: the copies, and the slots of ONE ingest upload and of at most one stream_group_s16_kernel and one stream_group_resample_kernel launch) and
// group_run_rounds (ONE order upload, the rounds, pos and steps), then group_drain (every entry's SessionOut around the call's ONE synchronisation).  The rounds see
// 16 kHz rings only.
struct GroupFeed { int member; const void* p; FeedPlan plan; };      // one entry of the call: its member, its samples (f32 or 16-bit, at the member's rate), its plan
struct GroupCall { std::vector<GroupFeed> fs; int32_t mem_kind = VOX_MEM_HOST; bool s16 = false, staged = false, any_rate = false, peek = false; };      // staged: host 16-bit samples pass through g->s16_stage; peek: every entry is planned as a finish (vox_stream_group_peek)
typedef std::vector<std::pair<int, int>> GroupDue;      // (ticks due in this pass, member)
static int32_t group_plan_entries(const vox_stream_group* g, const vox_stream_feed* feeds, int32_t n_feeds, GroupCall* call) {
    unsigned seen = 0; int pages = 0; call->fs.reserve((size_t)n_feeds);
    for (int k = 0; k < n_feeds; k++) {
        const vox_stream_feed& f = feeds[k];
        ARGCHK(f.member >= 0 && f.member < g->n, "entry %d: member %d out of range (0..%d)", k, f.member, g->n - 1);
        ARGCHK(!((seen >> f.member) & 1u), "entry %d: member %d is fed twice in one call", k, f.member); seen |= 1u << f.member;
        char who[48]; snprintf(who, sizeof who, "entry %d: ", k);
        VOXCHK(entry_check(who, f.samples, f.n_samples, f.out_ids, f.cap)); ARGCHK(f.finish == 0 || f.finish == 1, "entry %d: finish must be 0 or 1", k);
        if (call->peek) ARGCHK(f.n_samples == 0 && f.finish == 0, "entry %d: a peek takes no samples and no finish flag (push first, then peek)", k);
        snprintf(who, sizeof who, "entry %d: member %d", k, f.member);
        GroupFeed gf{f.member, f.samples, FeedPlan{}};
        VOXCHK(feed_plan(g->mem[f.member].feed, g->m->cfg.reshape_factor, g->g.left, g->g.max_pos, f.n_samples, call->peek || f.finish != 0, f.cap, who, &gf.plan));
        call->any_rate |= g->mem[f.member].rate >= 0;
        call->fs.push_back(gf);
        if (g->paged) {      // the logical pages the entry's ticks enter: all of the call's are there, or the call is refused
            const int need = g->pool.need(f.member, gf.plan.target); pages += need;
            ARGCHK(pages <= g->pool.n_free(), "entry %d: member %d: the call needs %d new pages of the pool (this member %d), %d are free (a reset returns a member's pages)", k, f.member,
                   pages, need, g->pool.n_free());
            // a ring table has pool_pages entries: a member that would hold more than that needs more pages than the pool has -- the refusal above.  Stated here, and kept so
            ARGCHK(!g->endless || g->pool.held(f.member) + need <= g->pool.tab_len, "entry %d: member %d would hold %d pages, its table has %d entries", k, f.member, g->pool.held(f.member) + need,
                   g->pool.tab_len);
        }
    }
    return VOX_OK;
}
// behind every check of a paged group's call: the entries' pages are taken, in entry order, and their table entries go up in front of the call's rounds
static int32_t group_take_pages(vox_stream_group* g, const GroupCall& call) {
    for (const GroupFeed& e : call.fs) {
        int64_t q0, q1;
        if (!g->pool.take(e.member, e.plan.target, &q0, &q1)) return fail(VOX_ERR_INVALID, "internal: member %d: the planned pages are not free", e.member);
        VOXCHK(group_table_upload(g, e.member, q0, q1));
    }
    return VOX_OK;
}
// behind a committed call: the pages below each fed member's window go back (no later step reads them); their entries become -1 on the device as well, behind the
// call's rounds in stream order
static int32_t group_release_pages(vox_stream_group* g, const GroupCall& call) {
    for (const GroupFeed& e : call.fs) {
        int64_t q0, q1; g->pool.release_below_window(e.member, g->mem[e.member].feed.pos, &q0, &q1);
        VOXCHK(group_table_upload(g, e.member, q0, q1));
    }
    return VOX_OK;
}
// one pass: what fits into every fed member's rings.  f32 samples and the pad zeros go as copies; 16-bit samples (slot z of the conversion) and the 16 kHz samples a rate
// member's complete blocks give (slot z of the resampling, which reads what the conversion wrote) as the pass's ingest, in front of its rounds
static int32_t group_stage_pass(vox_stream_group* g, GroupCall& call, GroupDue* due, bool* idle) {
    const int R = g->m->cfg.reshape_factor; hipStream_t s = g->ctx->stream;
    bool any_pcm = false, any_rs = false; *idle = true; due->clear();
    GroupIngest* ing = nullptr;
    if (call.s16 || call.any_rate) { g->ingests.emplace_back(); ing = &g->ingests.back(); std::memset((void*)ing, 0, sizeof(GroupIngest)); }
    for (size_t z = 0; z < call.fs.size(); z++) {
        GroupFeed& e = call.fs[z]; FeedState& f = g->mem[e.member].feed; const bool rate = f.sr != 16000;
        float *ring16 = g->samples + (size_t)e.member * STREAM_SAMPLE_RING, *ring = rate ? f.in_ring : ring16; const int ring_n = rate ? f.in_ring_n : STREAM_SAMPLE_RING;
        const FeedPass q = feed_pass(f, e.plan, R, g->g.left, call.staged ? (size_t)STREAM_SAMPLE_RING : SIZE_MAX);
        if (!call.s16) { StreamSrc src; src.p = e.p; src.mem_kind = call.mem_kind; VOXCHK(ring_write_f32(s, ring, ring_n, q.in_w0, src, q.at, q.n_in)); }
        else if (q.n_in > 0) {
            const int16_t* v = (const int16_t*)e.p + q.at;
            if (call.staged) { int16_t* st = g->s16_stage + z * (size_t)STREAM_SAMPLE_RING; HIPCHK(hipMemcpyAsync(st, v, q.n_in * 2, hipMemcpyHostToDevice, s)); v = st; }
            ing->pcm[z] = StreamS16{v, (int)q.n_in, ring, ring_n - 1, (long)q.in_w0}; any_pcm = true;
        }
        if (rate && q.n16 > 0) {
            ing->rs[z] = StreamIngest{f.in_ring, f.in_ring_n - 1, (long)f.in_written, f.At, (int)f.rp.fft_in, (int)f.rp.fft_out, (int)f.rp.delay, ring16, (long)q.i0, (int)q.n16}; any_rs = true;
        }
        VOXCHK(ring_write_f32(s, ring16, STREAM_SAMPLE_RING, q.pad_w0, StreamSrc{}, 0, q.pad));
        if (q.ticks > 0) due->emplace_back(q.ticks, e.member);
        *idle &= q.idle();
    }
    if (any_pcm || any_rs) {
        HIPCHK(hipMemcpyAsync(g->d_ingest, ing, sizeof(GroupIngest), hipMemcpyHostToDevice, s));
        if (any_pcm) HIPCHK(launch_stream_group_s16(g->d_ingest->pcm, ing->pcm, (int)call.fs.size(), s));
        if (any_rs) HIPCHK(launch_stream_group_resample(g->d_ingest->rs, ing->rs, (int)call.fs.size(), STREAM_SAMPLE_RING - 1, s));
    }
    return VOX_OK;
}
// the pass's rounds: the members sorted by ticks due, descending; round r runs one tick of the first n_r = #{ticks > r} of them
// An endless group's member lists -- its token row, and the score and alternatives records it has -- hold fewer positions than the pass will reach: twice the positions
// until they do (at most the session limit), the old entries copied over, the descriptor pointed at the new arrays (stream_lists_grow's rule; a group runs no engine,
// so every point between two passes is a verification point).  A doubling synchronises once per list it has (list_grow: the token row, the score records, the
// alternatives records) and once for the descriptor upload -- up to four times, 12 doublings at the most in a session's life.  Never trimmed:
// vox_stream_group_info[5] counts them.
static int32_t group_lists_grow(vox_stream_group* g, int member, int need_pos) {
    GroupMember& me = g->mem[member]; hipStream_t s = g->ctx->stream;
    while (need_pos > me.lists_cap) {
        const int rows = (int)std::min<int64_t>(2LL * me.lists_cap, g->g.max_pos);
        ARGCHK(rows > me.lists_cap, "internal: member %d's lists of %d positions cannot grow", member, me.lists_cap);
        int tcap = me.lists_cap + 2;
        VOXCHK(list_grow((void**)&me.tokens, &tcap, rows + 2, 4, s));
        if (me.sc.dev) VOXCHK(me.sc.grow(rows + 2, s));
        if (me.al.dev) VOXCHK(me.al.grow(rows + 2, s));
        if (me.lv.dev) VOXCHK(me.lv.grow(rows + 2, s));
        me.lists_cap = rows;
        StreamMember& hm = g->h_mem[member]; hm.tokens = me.tokens;
        if (hm.scores) { hm.scores = me.sc.dev; hm.scores_cap = me.sc.cap; }
        if (hm.alts) { hm.alts = me.al.dev; hm.alts_cap = me.al.cap; }
        if (hm.levels) { hm.levels = me.lv.dev; hm.levels_cap = me.lv.cap; }
        VOXCHK(group_upload_members(g));      // synchronises
    }
    return VOX_OK;
}
// An endless group's RoPE rows for the ticks a pass is about to run: for every due member the decoder rows of positions pos .. pos + ticks - 1 into rows position & mask
// of ITS decoder ring, the R ticks encoder rows likewise -- made by rope_row_fill (vox_host_base.h: the row function of rope_rows_fill and so of every table and of
// vox_debug_rope_rows) from the factors computed once per group, in the rings'
// pinned host images, copied on the group's stream in front of the pass's rounds (two copies where a span wraps).  The images are not rewritten while the last pass's
// copies may be in flight: the event recorded behind them is waited for first (stream_rope_refill's rule) -- the host runs at most one pass ahead of the copies.
static int32_t group_rope_refill(vox_stream_group* g, const GroupDue& due) {
    const vox_model_cfg& c = g->m->cfg; hipStream_t s = g->ctx->stream; const int R = c.reshape_factor;
    if (g->rope.pending) { HIPCHK(hipEventSynchronize(g->rope.copied)); g->rope.pending = false; }
    auto fill = [&](float* host, float* dev, int member, int rows, int hd, const float* inv, int64_t first, int cnt, int64_t table_len) -> int32_t {
        const int half = hd / 2; const int64_t mask = rows - 1; const size_t base = (size_t)member * rows * hd;
        for (int i = 0; i < cnt; i++) { float* row = host + base + (size_t)((first + i) & mask) * hd; rope_row_fill(inv, half, first + i, table_len, row, row + half); }
        const int r0 = (int)(first & mask), k = std::min(cnt, rows - r0);
        HIPCHK(hipMemcpyAsync(dev + base + (size_t)r0 * hd, host + base + (size_t)r0 * hd, (size_t)k * hd * 4, hipMemcpyHostToDevice, s));
        if (cnt > k) HIPCHK(hipMemcpyAsync(dev + base, host + base, (size_t)(cnt - k) * hd * 4, hipMemcpyHostToDevice, s));      // the span wrapped
        return VOX_OK;
    };
    for (const std::pair<int, int>& d : due) {
        const int pos0 = g->mem[d.second].feed.pos, n = d.first;
        ARGCHK(n >= 1 && n <= GROUP_ROPE_ROWS, "internal: member %d: a pass of %d ticks, the RoPE rings hold %d rows per member", d.second, n, GROUP_ROPE_ROWS);
        VOXCHK(fill(g->rope.h_dec, g->rope.dec, d.second, GROUP_ROPE_ROWS, c.dec_head_dim, g->rope.inv_d.data(), pos0, n, ROPE_DEC_TABLE_LEN));
        VOXCHK(fill(g->rope.h_enc, g->rope.enc, d.second, GROUP_ROPE_ROWS * R, c.enc_head_dim, g->rope.inv_e.data(), (int64_t)g->g.RC + (int64_t)R * (pos0 - g->g.PC), R * n, ROPE_ENC_STREAM_TABLE_LEN));
    }
    HIPCHK(hipEventRecord(g->rope.copied, s)); g->rope.pending = true;
    return VOX_OK;
}
static int32_t group_run_rounds(vox_stream_group* g, const StreamWs& w, GroupDue& due) {
    if (g->endless) {
        for (const std::pair<int, int>& d : due) VOXCHK(group_lists_grow(g, d.second, g->mem[d.second].feed.pos + d.first));
        VOXCHK(group_rope_refill(g, due));
    }
    std::stable_sort(due.begin(), due.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first > b.first; });
    g->orders.emplace_back(); std::array<int, GROUP_MAX>& ord = g->orders.back(); ord.fill(0);
    for (size_t i = 0; i < due.size(); i++) ord[i] = due[i].second;
    HIPCHK(hipMemcpyAsync(g->d_order, ord.data(), sizeof(int) * GROUP_MAX, hipMemcpyHostToDevice, g->ctx->stream));      // the pass's one order upload
    int n_r = (int)due.size();
    if (g->burst > 1) {      // a burst group: round k runs the next min(ticks still due, burst) ticks of every member that has one (group_burst_rounds); all ones: a plain round
        int dues[GROUP_MAX], b[GROUP_MAX];
        for (size_t i = 0; i < due.size(); i++) dues[i] = due[i].first;
        for (int k = 0; (n_r = group_burst_rounds(dues, (int)due.size(), g->burst, k, b)) > 0; k++) {
            if (b[0] == 1) VOXCHK(group_round(g, w, n_r)); else VOXCHK(group_burst_round(g, w, n_r, b));
        }
    } else for (int r = 0; r < due[0].first; r++) {
        while (due[(size_t)n_r - 1].first <= r) n_r--;
        VOXCHK(group_round(g, w, n_r));
    }
    for (const std::pair<int, int>& d : due) { g->mem[d.second].feed.pos += d.first; g->mem[d.second].steps += (uint64_t)d.first; }
    return VOX_OK;
}
// keep (a peek): the ring rows and the state blocks go back in front of the synchronisation, the records go to peek_scores[k] (null: nowhere)
static int32_t group_drain(vox_stream_group* g, vox_stream_feed* feeds, const GroupCall& call, const StreamKeepParams* keep, vox_token_score* const* peek_scores) {
    hipStream_t s = g->ctx->stream;
    std::vector<SessionOut> outs;
    for (size_t k = 0; k < call.fs.size(); k++) {
        GroupMember& me = g->mem[call.fs[k].member];
        outs.push_back(SessionOut{&me.feed, &me.sc, &me.al, &me.lv, g->h_mem[call.fs[k].member].tokens, feeds[k].out_ids, call.fs[k].plan.due, call.peek, peek_scores ? peek_scores[k] : nullptr});
        VOXCHK(outs.back().enqueue(s));
    }
    if (keep) HIPCHK(launch_stream_keep(*keep, 1, s));
    HIPCHK(hipStreamSynchronize(s));      // the call's one synchronisation: every fed member's ids and records land
    g->orders.clear(); g->ingests.clear(); g->bdescs.clear();
    for (size_t k = 0; k < call.fs.size(); k++) {
        outs[k].settle();
        feeds[k].n_ids = outs[k].due; if (feeds[k].finish) outs[k].feed->finished = true;      // (a peek's entries carry no finish flag)
    }
    return VOX_OK;
}
// the passes: write what fits into every fed member's rings, run the rounds that became due, repeat (a push may be larger than the rings; a peek is one pass)
static int32_t group_passes(vox_stream_group* g, GroupCall& call) {
    StreamWs w; stream_ws_carve(g->m, g->n, g->ws, &w, g->burst); GroupDue due;
    for (int pass = 0;; pass++) {
        const GroupFeed* open = nullptr; bool idle = false;
        for (const GroupFeed& e : call.fs) if (!open && feed_open(g->mem[e.member].feed, e.plan)) open = &e;
        if (!open) return VOX_OK;
        if (call.peek && pass > 0) { char who[24]; snprintf(who, sizeof who, "member %d", open->member); return peek_second_pass(who); }
        VOXCHK(group_stage_pass(g, call, &due, &idle));
        if (idle) return fail(VOX_ERR_INVALID, "internal: stream group stalled");
        if (!due.empty()) VOXCHK(group_run_rounds(g, w, due));
    }
}
// behind the checks and the reservations: the save of a peek, the passes, the drain
static int32_t group_body(vox_stream_group* g, vox_stream_feed* feeds, GroupCall& call, const StreamKeepParams* keep, vox_token_score* const* peek_scores) {
    if (keep) {
        g->orders.emplace_back(); std::array<int, GROUP_MAX>& slots = g->orders.back(); slots.fill(0);      // (alive until the synchronisation, as a pass's order)
        for (size_t k = 0; k < call.fs.size(); k++) slots[k] = call.fs[k].member;
        HIPCHK(hipMemcpyAsync(g->keep.p, slots.data(), sizeof(int) * GROUP_MAX, hipMemcpyHostToDevice, g->ctx->stream));
        HIPCHK(launch_stream_keep(*keep, 0, g->ctx->stream));
    }
    VOXCHK(group_passes(g, call));
    return group_drain(g, feeds, call, keep, peek_scores);
}
namespace { struct GroupMark { FeedState::Mark feed; uint64_t steps; }; }      // what a peek takes back of a member (the slab does not grow, its tap count lives in its state block)
static int32_t group_run(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, GroupCall& call, vox_token_score* const* peek_scores) {
    ARGCHK(g && (feeds || n_feeds == 0), "null argument"); ARGCHK(n_feeds >= 0 && n_feeds <= g->n, "%d entries for a group of %d members", n_feeds, g->n);
    ARGCHK(call.mem_kind == VOX_MEM_HOST || call.mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", call.mem_kind);
    vox_model* m = g->m; const vox_model_cfg& c = m->cfg; const int R = c.reshape_factor; hipStream_t s = g->ctx->stream;
    call.staged = call.s16 && call.mem_kind == VOX_MEM_HOST;
    VOXCHK(group_plan_entries(g, feeds, n_feeds, &call));      // every check before anything changes: a refused call can be repeated
    const int n = (int)call.fs.size(); int keep_rows = 0;
    if (call.peek && n == 0) return VOX_OK;
    if (call.peek) {      // the bound on every entry's ticks; the keep's rows from the largest
        int T = 0;
        for (const GroupFeed& e : call.fs) { char who[24]; snprintf(who, sizeof who, "member %d: ", e.member); int t; VOXCHK(peek_max_ticks(g->mem[e.member].feed, R, e.plan.due, who, &t)); T = std::max(T, t); }
        keep_rows = std::min(g->g.cap, R * T);
    }
    VOXCHK(ctx_bind(g->ctx));
    if (call.staged && !g->s16_stage && n > 0) {      // STREAM_SAMPLE_RING staged samples per entry and pass
        const size_t nb = (size_t)g->n * STREAM_SAMPLE_RING * 2;
        HIPCHK(hipMalloc((void**)&g->s16_stage, nb)); g->bytes += nb;
    }
    if (call.peek) VOXCHK(keep_reserve(g->keep, GROUP_MAX + (size_t)n * stream_keep_floats(c.enc_layers, c.enc_heads, c.enc_head_dim, keep_rows), &g->bytes, s, "group"));
    if (m->pw_pend_rows > 0) VOXCHK(pw_sync(m));
    if (!g->ada) VOXCHK(vox_model_set_t_embed(m, g->t_embed.data()));      // (a delay per member: the round reads the group's own scales, the model's t_embed stays what it is)
    for (GroupFeed& e : call.fs) g->mem[e.member].feed.n_pushed += (int64_t)e.plan.n;
    PagePool::Mark pool_was; std::vector<int> took;
    if (g->paged) { if (call.peek) { pool_was = g->pool.mark(); for (const GroupFeed& e : call.fs) took.push_back(e.member); } VOXCHK(group_take_pages(g, call)); }
    if (!call.peek) { VOXCHK(group_body(g, feeds, call, nullptr, nullptr)); return g->paged ? group_release_pages(g, call) : VOX_OK; }
    // a peek: the peeking members are the ring keep's slots, their numbers the first 16 ints of the save area
    const StreamKeepParams keep = ring_keep(c, g->d_mem, reinterpret_cast<const int*>(g->keep.p), n, keep_rows, g->g.cap, g->keep.p + GROUP_MAX);
    std::vector<GroupMark> was; for (const GroupFeed& e : call.fs) was.push_back(GroupMark{g->mem[e.member].feed.mark(), g->mem[e.member].steps});
    const uint64_t rounds_was[3] = {g->burst_rounds, g->burst_member_ticks, g->plain_rounds};      // (a peek's rounds are not counted, as a solo burst stream's)
    const int32_t r = group_body(g, feeds, call, &keep, peek_scores);
    g->burst_rounds = rounds_was[0]; g->burst_member_ticks = rounds_was[1]; g->plain_rounds = rounds_was[2];
    if (r != VOX_OK) { (void)launch_stream_keep(keep, 1, s); (void)hipStreamSynchronize(s); g->orders.clear(); g->ingests.clear(); g->bdescs.clear(); }      // a failed tail is taken back as well
    for (int k = 0; k < n; k++) { GroupMember& me = g->mem[call.fs[(size_t)k].member]; me.feed.rewind(was[(size_t)k].feed); me.steps = was[(size_t)k].steps; }
    if (g->paged) {      // the tail's pages go back: the pool, the tables and the peak are what they were (the device entries too, behind the tail in stream order)
        std::vector<int64_t> ends; for (int member : took) ends.push_back(g->pool.mem[(size_t)member].end);
        g->pool.undo(pool_was, took);
        for (size_t k = 0; k < took.size(); k++) (void)group_table_upload(g, took[k], g->pool.mem[(size_t)took[k]].end, ends[k]);
    }
    return r;
}
extern "C" int32_t vox_stream_group_advance(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, int32_t mem_kind) {
    GroupCall call; call.mem_kind = mem_kind; return group_run(g, feeds, n_feeds, call, nullptr);
}
extern "C" int32_t vox_stream_group_advance_s16(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, int32_t mem_kind) {
    GroupCall call; call.mem_kind = mem_kind; call.s16 = true; return group_run(g, feeds, n_feeds, call, nullptr);
}
extern "C" int32_t vox_stream_group_peek(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, vox_token_score* const* scores_or_null) {
    GroupCall call; call.peek = true; return group_run(g, feeds, n_feeds, call, scores_or_null);
}
extern "C" int32_t vox_stream_group_set_scores(vox_stream_group* g, int32_t member, int32_t on) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1); ARGCHK(on == 0 || on == 1, "on must be 0 or 1");
    VOXCHK(ctx_bind(g->ctx));
    ScoreState& sc = g->mem[member].sc;
    if (on) { char whose[24]; snprintf(whose, sizeof whose, "member %d's", member); VOXCHK(sc.alloc(g->endless ? g->mem[member].lists_cap : g->g.max_pos, whose)); }      // the group's logits rows are there already: a member needs its records alone
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    g->h_mem[member].scores = on ? sc.dev : nullptr; g->h_mem[member].scores_cap = on ? sc.cap : 0;
    VOXCHK(group_upload_members(g));
    g->n_scored += (on != 0) - (int)sc.on; sc.on = on != 0;
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_scores(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_token_score* out) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    return g->mem[member].sc.read(g->mem[member].feed.ids_out, first_id, n, out);
}
extern "C" int32_t vox_stream_group_set_levels(vox_stream_group* g, int32_t member, int32_t on) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1); ARGCHK(on == 0 || on == 1, "on must be 0 or 1");
    VOXCHK(ctx_bind(g->ctx));
    LevelState& lv = g->mem[member].lv;
    if (on) { char whose[24]; snprintf(whose, sizeof whose, "member %d's", member); VOXCHK(lv.alloc(g->endless ? g->mem[member].lists_cap : g->g.max_pos, whose)); }
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    StreamMember& hm = g->h_mem[member]; const StreamMember was = hm;
    hm.levels = on ? lv.dev : nullptr; hm.levels_cap = on ? lv.cap : 0;
    const int32_t r = group_upload_members(g);
    if (r != VOX_OK) { hm = was; return r; }      // a failed upload leaves the host descriptor with the counter: n_leveled gates the round's launch
    g->n_leveled += (on != 0) - (int)lv.on; lv.on = on != 0;
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_levels(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_tick_level* out) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    return g->mem[member].lv.read(g->mem[member].feed.ids_out, first_id, n, out);
}
extern "C" int32_t vox_stream_group_quiet(const vox_stream_group* g, int32_t member, float peak_below, int32_t* ticks) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    return g->mem[member].lv.quiet(g->mem[member].feed.ids_out, peak_below, ticks);
}
extern "C" int32_t vox_stream_group_set_alternatives(vox_stream_group* g, int32_t member, int32_t k) {
    ARGCHK(g, "null group"); ARGCHK(k >= 0 && k <= VOX_MAX_ALTERNATIVES, "k %d out of range (0..%d)", k, VOX_MAX_ALTERNATIVES);      // (k before the handle is read)
    ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    VOXCHK(ctx_bind(g->ctx));
    AltsState& al = g->mem[member].al;
    if (k > 0) { char whose[24]; snprintf(whose, sizeof whose, "member %d's", member); VOXCHK(al.alloc(g->endless ? g->mem[member].lists_cap : g->g.max_pos, whose)); }      // (the group's logits rows are there already)
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    StreamMember& hm = g->h_mem[member]; const StreamMember was = hm;
    hm.alts = k > 0 ? al.dev : nullptr; hm.alts_cap = k > 0 ? al.cap : 0; hm.alts_k = k;
    const int32_t r = group_upload_members(g);
    if (r != VOX_OK) { hm = was; return r; }      // a failed upload leaves the host descriptor with the counters: n_alts gates the round's launch
    g->n_alts += (k > 0) - (al.k > 0); al.k = k;
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_alternatives(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_token_alts* out) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    return g->mem[member].al.read(g->mem[member].feed.ids_out, first_id, n, out);
}
extern "C" int32_t vox_stream_group_peeked_alternatives(const vox_stream_group* g, int32_t member, vox_token_alts* out, int32_t cap, int32_t* n) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    return g->mem[member].al.read_peeked(out, cap, n);
}
extern "C" int32_t vox_debug_stream_group_tap_arm(vox_stream_group* g, int32_t member, int32_t max_rows) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    ARGCHK(max_rows > 0 && max_rows <= 65536, "max_rows %d out of range (1..65536)", max_rows); VOXCHK(ctx_bind(g->ctx));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    StreamMember& me = g->h_mem[member];
    if (me.tap) { (void)hipFree(me.tap); me.tap = nullptr; me.tap_max = 0; }
    HIPCHK(hipMalloc((void**)&me.tap, (size_t)max_rows * g->m->cfg.vocab * 4)); me.tap_max = max_rows;
    HIPCHK(hipMemsetAsync(me.state + STRM_TAP_ROWS, 0, 4, g->ctx->stream));
    return group_upload_members(g);
}
extern "C" int32_t vox_debug_stream_group_tap_fetch(vox_stream_group* g, int32_t member, float* out, int32_t* rows) {
    ARGCHK(g && out && rows, "null argument"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    StreamMember& me = g->h_mem[member];
    ARGCHK(me.tap, "no tap to fetch for member %d (vox_debug_stream_group_tap_arm)", member); VOXCHK(ctx_bind(g->ctx));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    int n = 0; HIPCHK(hipMemcpy(&n, me.state + STRM_TAP_ROWS, 4, hipMemcpyDeviceToHost));
    const int k = std::min(n, me.tap_max);
    if (k > 0) HIPCHK(hipMemcpy(out, me.tap, (size_t)k * g->m->cfg.vocab * 4, hipMemcpyDeviceToHost));
    *rows = n;
    (void)hipFree(me.tap); me.tap = nullptr; me.tap_max = 0;
    return group_upload_members(g);
}

// ---- snapshot and resume of a member (vox_stream_group_snapshot, vox_stream_group_restore): the solo stream's two functions on the member seen as a SnapSession --
// its slice of the slab as flat planes, or its row of the page table (a ring table in an endless group).  The blob does not know where it came from.
static SnapSession group_session(vox_stream_group* g, int i) {
    const vox_model_cfg& c = g->m->cfg; GroupMember& me = g->mem[(size_t)i]; const StreamMember& hm = g->h_mem[(size_t)i];
    static thread_local char who[32]; snprintf(who, sizeof who, "member %d", i);
    SnapSession ss{}; ss.m = g->m; ss.ctx = g->ctx; ss.t_embed = &group_t_embed(g, i); ss.feed = &me.feed; ss.sc = &me.sc; ss.al = &me.al; ss.lv = &me.lv; ss.gain = hm.gain;
    ss.tokens = hm.tokens; ss.samples = const_cast<float*>(hm.samples); ss.state = hm.state; ss.h_state = me.h_state; ss.cap = g->g.cap; ss.PC = g->g.PC; ss.max_pos = g->g.max_pos; ss.who = who;
    ss.enc.cache_k = hm.kring; ss.enc.cache_v = hm.vring; ss.enc.layers = c.enc_layers; ss.enc.heads = c.enc_heads; ss.enc.hd = c.enc_head_dim;
    ss.enc.layout = vox::SNAP_RING; ss.enc.cap = g->g.cap; ss.enc.layer_stride = g->ring_layer; ss.enc.head_stride = (size_t)g->g.cap * c.enc_head_dim;
    ss.dec.layers = c.dec_layers; ss.dec.heads = c.dec_kv_heads; ss.dec.hd = c.dec_head_dim; ss.dec.layer_stride = g->layer_stride;
    if (g->paged) {
        ss.dec.cache_k = g->dec_k; ss.dec.cache_v = g->dec_v; ss.dec.layout = g->endless ? vox::SNAP_PAGED_RING : vox::SNAP_PAGED; ss.dec.head_stride = (size_t)g->pool.page_rows * c.dec_head_dim;
        ss.dec.tab = g->d_tab + (size_t)i * g->pool.tab_len; ss.dec.shift = g->pool.shift; ss.dec.tab_len = g->pool.tab_len; ss.dec.page_floats = g->page_floats; ss.dec.kv_bf16 = g->kv_bf16 ? 1 : 0;
    } else {
        ss.dec.cache_k = g->dec_k + (size_t)i * g->seq_stride; ss.dec.cache_v = g->dec_v + (size_t)i * g->seq_stride; ss.dec.layout = vox::SNAP_FLAT; ss.dec.head_stride = (size_t)g->g.max_pos * c.dec_head_dim;
    }
    return ss;
}
// in front of a launch on a paged member: every table entry the blob's decoder rows touch names a page of the pool (the host mirror of the member's table)
static int32_t group_snap_pages_check(const vox_stream_group* g, int i, const vox_snap::SnapHeader& h) {
    if (!g->paged) return VOX_OK;
    int bad = 0;
    if (!snapshot_kv_pages_ok(g->pool.mem[(size_t)i].tab.data(), g->endless ? vox::SNAP_PAGED_RING : vox::SNAP_PAGED, g->pool.shift, g->pool.tab_len, h.D - h.Wd, h.D, g->pool.pool_pages, &bad))
        return fail(VOX_ERR_INVALID, "internal: member %d: logical page %d of its window is %d, outside the pool's %d pages", i, bad, g->pool.at(i, bad), g->pool.pool_pages);
    return VOX_OK;
}
extern "C" int32_t vox_stream_group_snapshot_size(const vox_stream_group* g, int32_t member, size_t* nbytes) {
    ARGCHK(g && nbytes, "null argument"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    ARGCHK(!g->mem[(size_t)member].feed.finished, "member %d is finished: a reset starts its next utterance", member);
    vox_snap::SnapHeader h; session_snap_header(group_session(const_cast<vox_stream_group*>(g), member), &h);
    *nbytes = (size_t)h.total_bytes; return VOX_OK;
}
extern "C" int32_t vox_stream_group_snapshot(vox_stream_group* g, int32_t member, void* blob, size_t cap, size_t* nbytes, int32_t mem_kind) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    VOXCHK(ctx_bind(g->ctx));
    const SnapSession ss = group_session(g, member);
    vox_snap::SnapHeader h; session_snap_header(ss, &h); VOXCHK(group_snap_pages_check(g, member, h));
    return session_snapshot(ss, blob, cap, nbytes, mem_kind);
}
// The member becomes the blob's session: its rate from the blob (as vox_stream_group_reset_rate sets it), the blob's gain.  A paged member is planned like an advance:
// the pages it holds now count as free, the pages vox_stream_group_pages_for(D) names are needed -- a pool without room refuses, and the group is untouched.
extern "C" int32_t vox_stream_group_restore(vox_stream_group* g, int32_t member, const void* blob, size_t nbytes, int32_t mem_kind) {
    ARGCHK(g, "null group"); ARGCHK(member >= 0 && member < g->n, "member %d out of range (0..%d)", member, g->n - 1);
    VOXCHK(ctx_bind(g->ctx));
    GroupMember& me = g->mem[(size_t)member]; hipStream_t s = g->ctx->stream;
    // ---- every check, nothing changed
    vox_snap::SnapHeader h; VOXCHK(session_restore_check(group_session(g, member), blob, nbytes, mem_kind, &h));
    int ring_n = 0;
    if (h.sample_rate != 16000) { ResamplePlan rp; size_t rs_bytes; VOXCHK(stream_rate_plan(h.sample_rate, &rp, &rs_bytes, &ring_n)); }
    ARGCHK(h.sec_len[vox_snap::SEC_IN_SAMPLES] == (uint64_t)std::min<int64_t>(h.in_written, ring_n) * 4, "snapshot: an input ring section of %llu bytes for a ring of %d samples",
           (unsigned long long)h.sec_len[vox_snap::SEC_IN_SAMPLES], ring_n);
    int first = 0, n_pages = 0;
    if (g->paged) {
        pages_held(h.D, g->pool.page_rows, g->pool.window, &first, &n_pages);
        ARGCHK(n_pages <= g->pool.held(member) + g->pool.n_free(), "member %d: the restore needs %d pages of the pool, %d are free (the %d the member holds now included; a reset returns a member's pages)",
               member, n_pages, g->pool.held(member) + g->pool.n_free(), g->pool.held(member));
    }
    HIPCHK(hipStreamSynchronize(s));
    VOXCHK(group_member_set_rate(g, member, h.sample_rate));      // refused: the member, its rate and its state are as they were
    // ---- from here on the member is the blob's session
    int32_t r = VOX_OK;
    auto body = [&]() -> int32_t {
        if (g->endless) VOXCHK(group_lists_grow(g, member, h.D));
        if (g->paged) {
            int64_t q0, q1, t0, t1;
            g->pool.release_all(member, &q0, &q1); g->pool.start_at(member, first);
            if (!g->pool.take(member, h.D, &t0, &t1)) return fail(VOX_ERR_INVALID, "internal: member %d: the planned pages are not free", member);
            VOXCHK(group_table_upload(g, member, q0, q1)); VOXCHK(group_table_upload(g, member, t0, t1));
            VOXCHK(group_snap_pages_check(g, member, h));
        }
        g->h_mem[(size_t)member].gain = h.gain;
        VOXCHK(group_upload_members(g));
        VOXCHK(session_restore_check_ring(group_session(g, member), h));
        return session_restore_payload(group_session(g, member), h, blob, mem_kind);
    };
    r = body();
    if (r != VOX_OK) { (void)hipStreamSynchronize(s); (void)group_member_seed(g, member); return r; }      // a failure half way: the member is a fresh session, not half of two
    me.steps = 0;
    return VOX_OK;
}

// ---- debug: the sample front ends on their own (tests).  form 0: the single clip's (clip_front_end); form 1: the batch drivers' (group_peak_scales when norm_group is
// given, front_end_units with the drivers' host packing and device pointers).  Every unit's scale and [128][T_i] log-mel come back to the host.
extern "C" int32_t vox_debug_front_end(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group, int32_t form,
                                       int32_t mem_kind, float* out_scales, float* const* out_mels, int32_t* out_T) {
    ARGCHK(m && samples && n_samples && out_scales && out_mels && out_T, "null argument");
    ARGCHK(form == 0 || form == 1, "bad form %d (0 single clip, 1 batch)", form); ARGCHK(mem_kind == VOX_MEM_HOST || mem_kind == VOX_MEM_DEVICE, "bad mem_kind %d", mem_kind);
    ARGCHK(n > 0 && n <= 128, "unit count %d out of range (1..128)", n);
    ARGCHK(form == 1 || (n == 1 && !norm_group), "the single-clip front end takes one unit and no norm_group");
    for (int i = 0; i < n; i++) ARGCHK(samples[i] && n_samples[i] > 0 && n_samples[i] <= ((size_t)1 << 30) && out_mels[i], "empty audio or null output in slot %d", i);
    ARGCHK(m->cfg.n_mels == 128, "the log-mel front-end produces 128 bins; model expects %d", m->cfg.n_mels);
    VOXCHK(ctx_bind(m->ctx)); vox_ctx* cx = m->ctx; hipStream_t s = cx->stream;
    if (form == 0) {
        int T = 0; VOXCHK(clip_front_end(m, samples[0], n_samples[0], mem_kind, &T));
        HIPCHK(hipMemcpyAsync(out_scales, cx->d_scale, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(out_mels[0], m->d_mel, (size_t)128 * T * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s)); out_T[0] = T;
        return VOX_OK;
    }
    GroupScales gs; const float* const* smp = samples; int32_t mk = mem_kind;      // as transcribe_batch_one_session hands the units to the drivers
    if (norm_group) {
        VOXCHK(group_peak_scales(m, n, samples, n_samples, norm_group, mem_kind, gs));
        if (!gs.dev_s.empty()) { smp = gs.dev_s.data(); mk = VOX_MEM_DEVICE; }
    }
    const float* const* unit_scale = norm_group ? gs.scale_of.data() : nullptr;
    MelTables mt; VOXCHK(ctx_mel_tables(cx, &mt));
    std::vector<int> S, T, len, slot_of(n); std::vector<int32_t> caps(n, INT32_MAX); int Smax = 0;
    for (int i = 0; i < n; i++) slot_of[i] = i;
    VOXCHK(batch_lengths(m, n, smp, n_samples, caps.data(), slot_of.data(), T, S, len, &Smax));
    size_t mel_floats = 0, smp_total = 0; for (int i = 0; i < n; i++) { mel_floats += (size_t)128 * T[i]; smp_total += n_samples[i]; }
    DevBuf b_mel, b_scale, b_smp; BatchDrain drain{cx};
    HIPCHK(b_mel.alloc_pooled(cx, mel_floats * 4)); HIPCHK(b_scale.alloc_pooled(cx, (size_t)n * 4));
    if (mk == VOX_MEM_HOST) HIPCHK(b_smp.alloc_pooled(cx, smp_total * 4));
    std::vector<const float*> d_mels(n);
    VOXCHK(front_end_units(mt, 0, n, smp, n_samples, T.data(), unit_scale, mk == VOX_MEM_HOST ? b_smp.as<float>() : nullptr, b_mel.as<float>(), b_scale.as<float>(), d_mels.data(), s));
    for (int i = 0; i < n; i++) {
        HIPCHK(hipMemcpyAsync(out_scales + i, unit_scale ? unit_scale[i] : b_scale.as<float>() + i, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_mels[i], d_mels[i], (size_t)128 * T[i] * 4, hipMemcpyDeviceToHost, s)); out_T[i] = T[i];
    }
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
