"""Host side of the stream group (vox_stream_group): the exported symbols, the argument checks that need no device, the caps the Python wrapper hands to
vox_stream_group_advance, the CLI's refusals.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ("vox_stream_group_create", "vox_stream_group_advance", "vox_stream_group_reset", "vox_stream_group_info", "vox_stream_group_free",
                 "vox_debug_stream_group_tap_arm", "vox_debug_stream_group_tap_fetch")


def test_symbols_are_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for name in GROUP_SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr
    assert "vox_stream_feed;" in hdr and C.sizeof(pkg._lib.StreamFeed) == 40      # two ints, a pointer, a size, a pointer, two ints
    assert pkg._lib.StreamFeed.samples.offset == 8 and pkg._lib.StreamFeed.out_ids.offset == 24 and pkg._lib.StreamFeed.n_ids.offset == 36


def test_bad_arguments_are_refused_before_any_device_use(pkg):
    L = pkg.lib(); INVALID = 1
    out = C.c_void_p(); t = np.zeros(8, np.float32); n = C.c_int32(); info = (C.c_int64 * 8)(); feed = pkg._lib.StreamFeed()

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    # without a model there is no group (a machine without a GPU cannot load one): create can only be refused, and says why
    assert "null" in refused(L.vox_stream_group_create(None, t.ctypes.data, 4, None, 0, 0, C.byref(out)))
    for bad in (0, -1, 17, 1 << 20):
        assert "n_members" in refused(L.vox_stream_group_create(None, t.ctypes.data, bad, None, 0, 0, C.byref(out)))
    assert out.value is None
    assert "null" in refused(L.vox_stream_group_advance(None, C.byref(feed), 1, 0))
    assert "null" in refused(L.vox_stream_group_reset(None, 0, 1.0))
    assert "null" in refused(L.vox_stream_group_info(None, 0, info))
    assert "null" in refused(L.vox_debug_stream_group_tap_arm(None, 0, 4))
    assert "null" in refused(L.vox_debug_stream_group_tap_fetch(None, 0, None, C.byref(n)))
    assert L.vox_stream_group_free(None) == 0      # like vox_stream_free: freeing nothing is fine


class _FakeLib:
    """The library with the two group calls the wrapper's advance makes replaced: info answers from a table, advance records the entries it was handed."""

    def __init__(self, real, state):
        self._real = real; self.state = state; self.calls = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def vox_stream_group_info(self, h, member, out):
        out[0], out[2] = self.state[member]      # samples pushed, ids handed out
        return 0

    def vox_stream_group_advance(self, h, feeds, n, mem_kind):
        self.calls.append([(feeds[i].member, feeds[i].finish, feeds[i].n_samples, feeds[i].cap) for i in range(n)])
        for i in range(n):
            feeds[i].n_ids = 0
        return 0


def test_wrapper_sizes_every_cap_from_the_schedule(pkg, monkeypatch):
    gguf = sys.modules[pkg.__name__ + ".gguf"]
    state = {0: (0, 0), 1: (50000, 17), 2: (2560 * 7 + 39, 7), 5: (0, 0)}
    fake = _FakeLib(pkg.lib(), state)
    monkeypatch.setattr(gguf, "lib", lambda: fake)
    g = object.__new__(pkg.LiveStreamGroup); g.h = None; g.n_members = 6; g.model = None; g._tap_max = {}
    feeds = {0: np.zeros(40, np.float32), 1: np.zeros(70000, np.float32), 2: np.zeros(1, np.float32), 5: np.zeros(0, np.float32)}
    out = g.advance(feeds, finish=(1, 5))
    assert set(out) == {0, 1, 2, 5} and all(v.size == 0 for v in out.values())
    (call,) = fake.calls
    assert [c[0] for c in call] == [0, 1, 2, 5] and [c[1] for c in call] == [0, 1, 0, 1] and [c[2] for c in call] == [40, 70000, 1, 0]
    for member, finish, n, cap in call:
        pushed, had = state[member]
        due = pkg.stream_schedule(pushed + n, finished=bool(finish))[1] - had
        assert cap == max(due, 1), (member, cap, due)      # (an entry with nothing due still hands over a one-id buffer)
    assert [c[3] for c in call] == [1, pkg.stream_schedule(120000, finished=True)[1] - 17, 1, 8]
    g2 = object.__new__(pkg.LiveStreamGroup); g2.h = None; g2.n_members = 2; g2.model = None; g2._tap_max = {}
    with pytest.raises(ValueError, match="member 3"):
        g2.advance({3: np.zeros(4, np.float32)})
    assert len(fake.calls) == 1      # refused before the library was called


def _cli(*args):
    cli = os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "cli.py")
    return subprocess.run([sys.executable, cli, "-a", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, needle", [
    (("--live-group", "4"), "--live-group applies with --live"),
    (("--live", "--live-group", "1"), "2..16"),
    (("--live", "--live-group", "17"), "2..16"),
    (("--live", "--live-group", "-3"), "2..16"),
    (("--live", "--live-group", "4", "--gpus", "2"), "--live runs one file at a time on one GPU"),
    (("--live", "--live-group", "4", "--batch", "8"), "--live runs one file at a time on one GPU"),
    (("--live", "--live-group", "4", "--live-native-rate"), "--live-native-rate"),
])
def test_cli_refuses_live_group_misuse(args, needle):
    r = _cli(*args)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == ""
