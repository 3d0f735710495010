"""Host side of a stream group's capture-rate and 16-bit ingest (vox_stream_group_create_rates, vox_stream_group_reset_rate, vox_stream_group_advance_s16): the exported
symbols, the argument checks that need no device, the caps and the entry the Python wrapper picks per call.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE_SYMBOLS = ("vox_stream_group_create_rates", "vox_stream_group_reset_rate", "vox_stream_group_advance_s16")


def test_symbols_are_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for name in RATE_SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr
    assert C.sizeof(pkg._lib.StreamFeed) == 40      # the rate is member state, the format belongs to the call: the entry did not grow


def test_bad_arguments_are_refused_before_any_device_use(pkg):
    L = pkg.lib(); INVALID = 1
    out = C.c_void_p(); t = np.zeros(8, np.float32); feed = pkg._lib.StreamFeed(); rates = np.array([48000, 8000, 16000, 44100], np.uint32)

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    assert "null" in refused(L.vox_stream_group_create_rates(None, t.ctypes.data, 4, None, rates.ctypes.data, 0, 0, C.byref(out)))
    assert "null" in refused(L.vox_stream_group_create_rates(None, t.ctypes.data, 4, None, None, 0, 0, C.byref(out)))
    for bad in (0, -1, 17, 1 << 20):
        assert "n_members" in refused(L.vox_stream_group_create_rates(None, t.ctypes.data, bad, None, None, 0, 0, C.byref(out)))
    assert out.value is None
    assert "null" in refused(L.vox_stream_group_advance_s16(None, C.byref(feed), 1, 0))
    assert "null" in refused(L.vox_stream_group_reset_rate(None, 0, 1.0, 48000))
    assert "null" in refused(L.vox_stream_group_reset_rate(None, 0, 1.0, 0))


class _FakeLib:
    """The library with the group calls the wrapper's advance makes replaced: info answers from a table, both advance entries record what they were handed."""

    def __init__(self, real, state):
        self._real = real; self.state = state; self.calls = []; self.touched = []

    def __getattr__(self, name):
        self.touched.append(name)
        return getattr(self._real, name)

    def vox_stream_group_info(self, h, member, out):
        out[0], out[2] = self.state[member]      # samples pushed (at the member's rate), ids handed out
        return 0

    def _advance(self, entry, feeds, n, mem_kind):
        self.calls.append((entry, mem_kind, [(feeds[i].member, feeds[i].finish, feeds[i].n_samples, feeds[i].cap, feeds[i].samples) for i in range(n)]))
        for i in range(n):
            feeds[i].n_ids = 0
        return 0

    def vox_stream_group_advance(self, h, feeds, n, mem_kind):
        return self._advance("f32", feeds, n, mem_kind)

    def vox_stream_group_advance_s16(self, h, feeds, n, mem_kind):
        return self._advance("s16", feeds, n, mem_kind)


def _bare(pkg, n, rates=None):
    g = object.__new__(pkg.LiveStreamGroup); g.h = None; g.n_members = n; g.model = None; g._tap_max = {}
    if rates is not None:
        g._rates = dict(rates)
    return g


def test_wrapper_sizes_every_cap_from_the_members_rate_schedule(pkg, monkeypatch):
    gguf = sys.modules[pkg.__name__ + ".gguf"]
    rates = {0: 48000, 1: 8000}      # member 2: no entry, 16 kHz
    state = {0: (150000, 7), 1: (20000, 9), 2: (2560 * 7 + 39, 7)}
    fake = _FakeLib(pkg.lib(), state)
    monkeypatch.setattr(gguf, "lib", lambda: fake)
    g = _bare(pkg, 3, rates)
    assert [g.sample_rate(k) for k in range(3)] == [48000, 8000, 16000]
    n_new = {0: 9601, 1: 30000, 2: 2561}
    # float32 arrays: the f32 entry
    out = g.advance({k: np.zeros(n, np.float32) for k, n in n_new.items()}, finish=(1,))
    assert set(out) == {0, 1, 2}
    # int16 arrays only: the 16-bit entry, the arrays handed over as they are
    pcm = {k: np.full(n, k + 1, np.int16) for k, n in n_new.items()}
    g.advance(pcm, finish=(1,))
    # mixed: the f32 entry
    g.advance({0: pcm[0], 1: np.zeros(n_new[1], np.float32), 2: pcm[2]}, finish=(1,))
    # device pointers: dtype picks the entry
    g.advance({k: (4096 * (k + 1), n) for k, n in n_new.items()}, finish=(1,), device=True, dtype="s16")
    g.advance({k: (4096 * (k + 1), n) for k, n in n_new.items()}, finish=(1,), device=True)
    assert [(c[0], c[1]) for c in fake.calls] == [("f32", 0), ("s16", 0), ("f32", 0), ("s16", 1), ("f32", 1)]
    for entry, kind, call in fake.calls:
        assert [c[0] for c in call] == [0, 1, 2] and [c[1] for c in call] == [0, 1, 0] and [c[2] for c in call] == [n_new[k] for k in range(3)]
        for member, finish, n, cap, _ in call:
            pushed, had = state[member]
            due = pkg.stream_schedule(pushed + n, finished=bool(finish), sample_rate=g.sample_rate(member))[1] - had
            assert cap == max(due, 1), (entry, member, cap, due)
    caps = [c[3] for c in fake.calls[0][2]]
    # the rate matters: the same counts read at 16 kHz give other caps for both rate members
    assert caps[0] != max(pkg.stream_schedule(150000 + 9601)[1] - 7, 1) and caps[1] != max(pkg.stream_schedule(50000, finished=True)[1] - 9, 1)
    assert fake.calls[1][2][0][4] == pcm[0].ctypes.data      # int16 in place
    with pytest.raises(ValueError, match="dtype"):
        g.advance({0: np.zeros(4, np.float32)}, dtype="s16")
    assert len(fake.calls) == 5


def test_mixed_call_converts_int16_exactly(pkg, monkeypatch):
    gguf = sys.modules[pkg.__name__ + ".gguf"]
    seen = {}

    class Grab(_FakeLib):
        def _advance(self, entry, feeds, n, mem_kind):
            for i in range(n):
                seen[feeds[i].member] = np.ctypeslib.as_array((C.c_float * feeds[i].n_samples).from_address(feeds[i].samples)).copy()
            return super()._advance(entry, feeds, n, mem_kind)

    fake = Grab(pkg.lib(), {0: (0, 0), 1: (0, 0)})
    monkeypatch.setattr(gguf, "lib", lambda: fake)
    v = np.array([-32768, 32767, -1, 1, 0, 12345], np.int16)
    _bare(pkg, 2).advance({0: v, 1: np.ones(3, np.float32)})
    assert fake.calls[0][0] == "f32" and np.array_equal(seen[0].astype(np.float64) * 32768.0, v.astype(np.float64))


def test_a_16k_f32_advance_calls_info_and_advance_only(pkg, monkeypatch):
    gguf = sys.modules[pkg.__name__ + ".gguf"]
    fake = _FakeLib(pkg.lib(), {0: (0, 0), 1: (50000, 17)})
    monkeypatch.setattr(gguf, "lib", lambda: fake)
    _bare(pkg, 2).advance({0: np.zeros(40, np.float32), 1: np.zeros(70000, np.float32)}, finish=(1,))
    assert len(fake.calls) == 1 and fake.calls[0][0] == "f32"
    assert set(fake.touched) <= {"vox_stream_schedule"}      # host arithmetic for the caps, as before; nothing else of the library
