"""A delay per member of a stream group, without a GPU: the new symbols are in the header, in the library and in the Python binding; the argument refusals that come
before anything touches a device; create_stream_group's delays= and t_embeds= hand the library the same bits and refuse a count mismatch; --live-delays parsing and
the CLI's refusals."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vox_stream_group_create_t_embeds", "vox_stream_group_reset_t_embed", "vox_stream_group_t_embed", "vox_debug_resid_xf")


def test_the_symbols_are_in_the_header_the_library_and_the_binding(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    L = pkg.lib()
    for name in NEW:
        assert re.search(rf"\bint32_t {name}\s*\(", hdr), name
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES, name
    assert "vox_resid_xf_desc" in hdr


def test_argument_refusals_come_before_any_device_work(pkg):
    L = pkg.lib(); err = lambda: L.vox_last_error().decode()
    dummy = C.c_void_p(1)      # a model / group pointer that must never be dereferenced: every case fails on an argument checked before it is read
    te = np.zeros((16, 8), np.float32); p = te.ctypes.data_as(C.c_void_p); out = C.c_void_p()
    create = lambda m, t, n, o=C.byref(out), paged=0, page_rows=0, pool=0, endless=0, kv=0, burst=1, maxp=0: \
        L.vox_stream_group_create_t_embeds(m, t, n, None, None, 0, maxp, paged, page_rows, pool, endless, kv, burst, o)
    assert create(None, p, 3) == 1 and "null argument" in err()
    assert create(dummy, None, 3) == 1 and "null argument" in err()
    assert create(dummy, p, 3, o=None) == 1 and "null argument" in err()
    for n in (0, -1, 17):
        assert create(dummy, p, n) == 1 and "n_members" in err(), n
    for burst in (0, 17):
        assert create(dummy, p, 3, burst=burst) == 1 and "burst_ticks" in err()
    assert create(dummy, p, 3, paged=2) == 1 and "paged" in err()
    assert create(dummy, p, 3, page_rows=16) == 1 and "slab group" in err()      # paged 0 takes no page arguments
    assert create(dummy, p, 3, kv=1) == 1 and "slab group" in err()
    assert create(dummy, p, 3, paged=1, kv=2) == 1 and "kv_dtype" in err()
    assert create(dummy, p, 3, paged=1, endless=1, maxp=64) == 1 and "endless" in err()
    assert out.value is None
    assert L.vox_stream_group_reset_t_embed(None, 0, 1.0, 0, p) == 1 and "null group" in err()
    assert L.vox_stream_group_t_embed(None, 0, p, 8) == 1 and L.vox_stream_group_t_embed(dummy, 0, None, 8) == 1
    assert L.vox_debug_resid_xf(None, dummy, dummy, p, p, p, p, None, p, p, p) == 1 and "null argument" in err()


def test_delays_and_t_embeds_hand_over_the_same_bits(pkg, monkeypatch):
    gg = __import__("importlib").import_module(pkg.__name__ + ".gguf")
    D = 64; seen = []

    class Stub:
        def vox_stream_group_create_t_embeds(self, m, te, n, gains, rates, cap, maxp, paged, page_rows, pool, endless, kv, burst, out):
            seen.append((np.ctypeslib.as_array(C.cast(te, C.POINTER(C.c_float)), shape=(n, D)).copy(), n, paged, page_rows, pool, endless, kv, burst))
            return 0

    monkeypatch.setattr(gg, "lib", lambda: Stub())
    model = types.SimpleNamespace(h=C.c_void_p(1), config=types.SimpleNamespace(dec_dim=D), _caches=set())
    make = lambda *a, **kw: gg.Q4VoxtralModel.create_stream_group(model, *a, **kw)
    emb = pkg.TimeEmbedding(D)
    g = make(None, 3, delays=[2, 6, 10])
    h = make(None, 3, t_embeds=[emb.embed(2.0), emb.embed(6.0), emb.embed(10.0)], page_rows=16, burst=4)
    assert g.per_member and h.per_member and len(seen) == 2
    assert np.array_equal(seen[0][0].view(np.uint32), seen[1][0].view(np.uint32)) and (seen[0][0][0] != seen[0][0][2]).any()
    assert seen[0][1:] == (3, 0, 0, 0, 0, 0, 1) and seen[1][1:] == (3, 1, 16, 0, 0, 0, 4)
    for kw in (dict(delays=[2, 6]), dict(delays=[2, 6, 10, 14]), dict(t_embeds=[emb.embed(2.0)] * 2), dict(t_embeds=[np.zeros(D + 1, np.float32)] * 3), dict(delays=[])):
        with pytest.raises(ValueError):
            make(None, 3, **kw)
    with pytest.raises(ValueError):
        make(None, 3, delays=[2, 6, 10], t_embeds=[emb.embed(2.0)] * 3)
    assert len(seen) == 2      # a refused call reaches no library function


def test_live_delays_parsing(pkg):
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    assert cli.parse_live_delays("6,10,2", 3) == [6, 10, 2]
    assert cli.parse_live_delays(" 6 , 10 ", 2) == [6, 10]
    assert cli.parse_live_delays("8", 4) == [8, 8, 8, 8]
    for text, n in (("6,10", 3), ("6,10,2,4", 3), ("6,x", 2), ("", 2), ("6,,10", 3), ("6.5,2", 2), ("-1,2", 2)):
        with pytest.raises(ValueError):
            cli.parse_live_delays(text, n)


def test_cli_refuses_bad_live_delays(pkg, capsys):
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    base = ["--gguf", "none.gguf", "--tokenizer", "none.json", "-a", "a.wav", "-a", "b.wav"]
    for extra, needle in ((["--live-delays", "6,10"], "applies with --live-group"),
                          (["--live", "--live-delays", "6,10"], "applies with --live-group"),
                          (["--live", "--live-group", "3", "--live-delays", "6,10"], "2 delays for 3 members"),
                          (["--live", "--live-group", "2", "--live-delays", "6,ten"], "integers")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2 and needle in capsys.readouterr().err, extra
