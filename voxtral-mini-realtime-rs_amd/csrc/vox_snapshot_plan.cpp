// vox_snapshot_plan.cpp -- the session blob's host arithmetic behind the C ABI: vox_snapshot_describe, vox_snapshot_bytes_for (no device)
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the device-free host units: DESIGN.md, "Host units".  The arithmetic itself is vox_snapshot.h.)
#include "vox_host_base.h"
#include "vox_snapshot.h"

using namespace vox_host;
using namespace vox_snap;

extern "C" int32_t vox_snapshot_describe(const void* blob, size_t nbytes, vox_snapshot_info* out) {
    ARGCHK(blob && out, "null argument");
    SnapHeader h; char msg[256];
    if (!snap_parse(blob, nbytes, &h, msg, sizeof msg)) return fail(VOX_ERR_INVALID, "%s", msg);
    snap_info(h, out);
    return VOX_OK;
}

// the size function vox_stream_snapshot_size itself goes through: the blob of a session at decoder position `positions` that was pushed n_samples samples at
// sample_rate, with or without its record lists
extern "C" int32_t vox_snapshot_bytes_for(const vox_model_cfg* cfg, int64_t positions, uint32_t sample_rate, size_t n_samples, int32_t scores, int32_t alternatives, size_t* out) {
    ARGCHK(cfg && out, "null argument"); ARGCHK(sample_rate > 0, "bad sample rate 0"); ARGCHK(n_samples <= ((size_t)1 << 40), "sample count out of range");
    ARGCHK(positions >= SNAP_PREFIX_POS && positions < SNAP_POS_LIMIT, "positions %lld out of range (%d..2^24 - 1)", (long long)positions, SNAP_PREFIX_POS);
    ARGCHK(cfg->enc_layers > 0 && cfg->enc_heads > 0 && cfg->dec_layers > 0 && cfg->dec_kv_heads > 0 && cfg->enc_head_dim > 0 && cfg->dec_head_dim > 0 && cfg->enc_window >= 0 && cfg->reshape_factor > 0,
           "bad model configuration");
    ARGCHK((scores == 0 || scores == 1) && (alternatives == 0 || alternatives == 1), "scores and alternatives must be 0 or 1");
    SnapShape s; s.D = positions; s.E = (int64_t)cfg->reshape_factor * positions;
    int32_t pos_unused, ids_unused; size_t n16;
    VOXCHK(vox_stream_schedule_rate(n_samples, sample_rate, 0, &pos_unused, &ids_unused, &n16));
    s.n_written = (int64_t)n16;
    if (sample_rate != 16000) { ResamplePlan rp; size_t rs_bytes; int in_ring_n; VOXCHK(stream_rate_plan(sample_rate, &rp, &rs_bytes, &in_ring_n)); s.in_samples = (int64_t)std::min<size_t>(n_samples, (size_t)in_ring_n); }
    const int32_t ids = (int32_t)(positions - SNAP_PREFIX_POS);
    s.n_scores = scores ? ids : 0; s.n_alts = alternatives ? ids : 0;
    SnapHeader h{};
    *out = (size_t)snap_layout(*cfg, s, &h);
    return VOX_OK;
}
