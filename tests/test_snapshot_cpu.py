"""The session blob's host arithmetic (vox_snapshot_bytes_for, vox_snapshot_describe; include/voxtral_hip.h, SNAPSHOT AND RESUME): no device, no model file.

bytes_for is held to the format's formula written out here; describe to a header built here field by field from the layout the header comment documents -- so the
blob's layout cannot move without this file noticing -- and to its refusals, each of which leaves the output untouched."""
import ctypes as C
import struct

import numpy as np
import pytest

HEADER = 288
PREFIX_POS = 37
RING = 1 << 16


def _cfg(pkg, **kw):
    d = dict(enc_layers=3, enc_dim=128, enc_heads=2, enc_head_dim=64, enc_ffn=256, enc_window=750, dec_layers=2, dec_dim=256, dec_heads=4, dec_kv_heads=2, dec_head_dim=128,
             dec_ffn=512, dec_window=8192, vocab=512, n_mels=128, reshape_factor=4, t_cond_dim=32, rope_theta=1e6, norm_eps=1e-5)
    d.update(kw)
    return pkg._lib.ModelCfg(**d)


def _al(x):
    return (x + 15) // 16 * 16


def _sections(c, D, n16, n_in, n_scores, n_alts):
    """lengths of the nine sections by the documented formula"""
    E = c.reshape_factor * D
    We = min(E, c.enc_window); Wd = D if c.dec_window < 0 else min(D, c.dec_window)
    enc = c.enc_layers * c.enc_heads * We * c.enc_head_dim * 4; dec = c.dec_layers * c.dec_kv_heads * Wd * c.dec_head_dim * 4
    return [enc, enc, dec, dec, min(n16, RING) * 4, n_in * 4, (D + 1) * 4, n_scores * 16, n_alts * 72], We, Wd


def _formula(c, D, n16, n_in=0, scores=False, alts=False):
    ids = D - PREFIX_POS
    lens, _, _ = _sections(c, D, n16, n_in, ids if scores else 0, ids if alts else 0)
    o = HEADER
    for n in lens:
        o = _al(o + n)
    return o


def _bytes_for(pkg, c, D, sr=16000, n=0, scores=False, alts=False):
    out = C.c_size_t()
    code = pkg.lib().vox_snapshot_bytes_for(C.byref(c), D, sr, n, int(scores), int(alts), C.byref(out))
    return code, out.value


@pytest.mark.parametrize("D,what", [(100, "E below enc_window"), (187, "E just below enc_window (748)"), (188, "E above enc_window (752)"), (8191, "D below the window"),
                                    (8192, "D at the window"), (8193, "D above the window"), (20000, "far above both")])
def test_bytes_for_against_the_formula(pkg, D, what):
    c = _cfg(pkg)
    n = 2560 * (D - 30)      # (any count: at 16 kHz the ring section is min(n, 65 536) samples)
    for scores in (False, True):
        for alts in (False, True):
            code, got = _bytes_for(pkg, c, D, n=n, scores=scores, alts=alts)
            assert code == 0, pkg.lib().vox_last_error()
            assert got == _formula(c, D, n, 0, scores, alts), (what, scores, alts)
    assert _bytes_for(pkg, c, D, n=n, scores=True)[1] - _bytes_for(pkg, c, D, n=n)[1] == 16 * (D - 37)      # records on - off: one 16-byte record per id


def test_bytes_for_enc_window_exactly_and_no_dec_window(pkg):
    c = _cfg(pkg, enc_window=752)      # E = 4 D meets the window exactly at D = 188
    for D in (187, 188, 189):
        assert _bytes_for(pkg, c, D, n=1000) == (0, _formula(c, D, 1000))
    c = _cfg(pkg, dec_window=-1)       # no decoder window: every row
    assert _bytes_for(pkg, c, 9000, n=5) == (0, _formula(c, 9000, 5))
    assert _bytes_for(pkg, c, 37, n=0) == (0, _formula(c, 37, 0))      # a fresh session: the prefix rows, no samples, no ids


def test_bytes_for_a_rate_stream(pkg):
    c = _cfg(pkg)
    fi, fo, delay = pkg.resample_plan(48000, 16000)[:3]
    ring = 1
    while ring < 2 * fi + (1 << 15):
        ring *= 2
    for n in (0, 777, fi + 5, 3 * fi + 17, 40 * fi + 1):
        n16 = max(0, n // fi * fo - delay)
        assert _bytes_for(pkg, c, 60, sr=48000, n=n) == (0, _formula(c, 60, n16, min(n, ring))), n
    assert _bytes_for(pkg, c, 60, sr=48000, n=40 * fi + 1)[1] > _bytes_for(pkg, c, 60, sr=16000, n=(40 * fi + 1) // 3)[1]      # the input ring is in the blob


def test_bytes_for_refusals(pkg):
    c = _cfg(pkg); L = pkg.lib(); out = C.c_size_t()
    assert L.vox_snapshot_bytes_for(None, 100, 16000, 0, 0, 0, C.byref(out)) == 1 and L.vox_snapshot_bytes_for(C.byref(c), 100, 16000, 0, 0, 0, None) == 1
    assert _bytes_for(pkg, c, 36)[0] == 1 and b"positions 36" in L.vox_last_error()
    assert _bytes_for(pkg, c, 1 << 24)[0] == 1
    assert _bytes_for(pkg, c, 100, sr=0)[0] == 1
    assert L.vox_snapshot_bytes_for(C.byref(c), 100, 16000, 0, 2, 0, C.byref(out)) == 1


# ---- describe: a header built here from the documented layout
FMT = "<IIQ QQ fIq qq 4i 4i 8i 4i 9Q 9Q"


def _header(c, D=100, n16=5000, n_pushed=5000, in_written=0, n_in=0, sr=16000, scores=0, alts_k=0, token=7, gain=1.5, magic=0x50534f56, version=1, **over):
    ids = D - PREFIX_POS; n_scores = ids if scores else 0; n_alts = ids if alts_k else 0
    lens, We, Wd = _sections(c, D, n16, n_in, n_scores, n_alts)
    offs, o = [], HEADER
    for n in lens:
        offs.append(o); o = _al(o + n)
    f = dict(magic=magic, version=version, total=o, fp=0x1122334455667788, th=0x99, gain=gain, sr=sr, n_pushed=n_pushed, n_written=n16, in_written=in_written, D=D, E=c.reshape_factor * D,
             ids=ids, token=token, scores=scores, alts_k=alts_k, n_scores=n_scores, n_alts=n_alts, We=We, Wd=Wd, offs=offs, lens=lens)
    f.update(over)
    raw = struct.pack(FMT, f["magic"], f["version"], f["total"], f["fp"], f["th"], f["gain"], f["sr"], f["n_pushed"], f["n_written"], f["in_written"], f["D"], f["E"], f["ids"], f["token"],
                      f["scores"], f["alts_k"], f["n_scores"], f["n_alts"], c.enc_layers, c.enc_heads, c.enc_head_dim, c.enc_window, c.dec_layers, c.dec_kv_heads, c.dec_head_dim,
                      c.dec_window, c.vocab, c.reshape_factor, f["We"], f["Wd"], *f["offs"], *f["lens"])
    assert len(raw) == HEADER
    return raw, f


def _describe(pkg, raw, nbytes):
    """the header bytes alone, in a buffer of exactly their length: describe may read nothing behind them"""
    buf = np.frombuffer(raw, dtype=np.uint8).copy()
    info = pkg._lib.SnapshotInfo(); info.version = -99
    code = pkg.lib().vox_snapshot_describe(buf.ctypes.data, nbytes, C.byref(info))
    return code, info, (pkg.lib().vox_last_error() or b"").decode()


def test_describe_decodes_a_header(pkg):
    c = _cfg(pkg)
    raw, f = _header(c, D=300, n16=70000, n_pushed=70000, scores=1, alts_k=3)
    code, info, msg = _describe(pkg, raw, f["total"])
    assert code == 0, msg
    assert (info.version, info.sample_rate, info.token, info.total_bytes, info.fingerprint, info.t_embed_hash) == (1, 16000, 7, f["total"], 0x1122334455667788, 0x99)
    assert (info.positions, info.enc_position, info.ids, info.scores, info.alternatives, info.n_scores, info.n_alts) == (300, 1200, 263, 1, 3, 263, 263)
    assert (info.enc_rows, info.dec_rows, info.samples_pushed, info.samples_16k, info.samples_in) == (750, 300, 70000, 70000, 0) and info.gain == 1.5
    assert list(info.section_offset) == f["offs"] and list(info.section_bytes) == f["lens"]
    assert f["total"] == _bytes_for(pkg, c, 300, n=70000, scores=True, alts=True)[1]      # the two functions agree on the layout
    d = pkg.snapshot_info(np.frombuffer(raw + bytes(f["total"] - HEADER), dtype=np.uint8))
    assert d["positions"] == 300 and d["section_bytes"] == f["lens"]


def test_describe_refusals(pkg):
    c = _cfg(pkg)
    raw, f = _header(c)
    total = f["total"]

    def refused(raw, nbytes, text):
        code, info, msg = _describe(pkg, raw, nbytes)
        assert code == 1 and text in msg, (text, code, msg)
        assert info.version == -99      # the output is untouched

    refused(raw[:HEADER - 1], HEADER - 1, "shorter than the 288-byte header")      # a short header
    refused(raw[:16], 16, "shorter than")
    refused(_header(c, magic=0x50534f57)[0], total, "bad magic")
    refused(_header(c, version=2)[0], total, "format version 2")                    # a future version
    refused(raw, total - 1, "bytes, ")                                               # a truncated blob: total_bytes != nbytes
    refused(raw, total + 16, "bytes, ")
    offs = list(f["offs"]); offs[3] = offs[2] + 16                                   # decoder V starts inside decoder K
    refused(_header(c, offs=offs)[0], total, "overlaps")
    offs = list(f["offs"]); offs[8] = _al(total) + 16                                # the last section lies behind the end
    refused(_header(c, offs=offs)[0], total, "runs past")
    offs = list(f["offs"]); offs[6] = total - 16                                     # the tokens start inside the blob and run past its end
    refused(_header(c, offs=offs)[0], total, "runs past")
    offs = list(f["offs"]); offs[1] += 4
    refused(_header(c, offs=offs)[0], total, "16-byte boundary")
    lens = list(f["lens"]); lens[2] += 16
    refused(_header(c, lens=lens)[0], total, "its contents need")
    refused(_header(c, token=512)[0], total, "outside the vocabulary")               # a token >= vocab
    refused(_header(c, token=-1)[0], total, "outside the vocabulary")
    refused(_header(c, E=401)[0], total, "encoder position")
    refused(_header(c, We=399)[0], total, "do not follow from the positions")
    refused(_header(c, ids=101)[0], total, "ids handed out")
    refused(_header(c, gain=float("nan"))[0], total, "gain")
    assert pkg.lib().vox_snapshot_describe(None, total, C.byref(pkg._lib.SnapshotInfo())) == 1
    with pytest.raises(pkg.VoxError):
        pkg.snapshot_info(np.zeros(10, np.uint8))
