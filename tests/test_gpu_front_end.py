"""The sample front end, value by value: peak scale, virtual pad and log-mel of the single clip (vox_transcribe_audio's preamble, `form` 0 of vox_debug_front_end) and
of the batch drivers (front_end_units + the group peaks of vox_transcribe_batch_ex, `form` 1), against the float64 reference of tests/frontend_ref.py (pinned to the
CPU oracle and to the reference project's vectors by tests/test_frontend_ref.py).  The live stream's front end is held to the same reference in tests/test_gpu_stream.py.

Bars
 * log-mel: |gpu - ref64| <= 1e-4 on every value (the bar of test_log_mel_vs_oracle), near the floor as well: powers below 10^-6.5 are clamped, the f32 DFT
   noise power for |x| <= 0.95 lies four orders of magnitude below that.  Frames that see only the pad's zeros are at the floor (-0.625) EXACTLY.
 * scales: bit for bit float32(0.95) / float32(max|x|) (one correctly rounded f32 division), 1 below 1e-10; every unit of a group gets the group's.
 * so that the log-mel comparison is not floor against floor, every noise clip asserts that at least half of the reference values in the frames that overlap the clip
   lie more than 0.05 above the floor (the silent pad alone is 71 % of a 3 s clip's frames).
The worst errors are printed per form; DESIGN.md section 4 ("Sample front end against float64") records them.  The clip closest to the bar is the 3 s tone + 1e-2
noise: 9.9e-5 -- 440 Hz is exactly DFT bin 11, so in the neighbouring bins the tone cancels to nothing while the f32 running sums swing by ~30 / (k - 11); what is left
is the noise (amplitude ~0.2) plus the running sums' rounding.

That these tests can fail: the library was built with each of the value-only mutations below (none moves an address out of its buffer) and this module and the
front-end cases of tests/test_gpu_stream.py were run once per build on the MI355X (tiny model).  What failed:
 (a) launch_group_scale called with 0.9f instead of 0.95f: test_batch_front_end[True-host], [True-device] (group scales), test_silence_threshold[1e-10], [2e-10]
     (the group of two); the ungrouped cases pass, as they must.
 (b) mel_kernel skips the scale multiply for j == 0: NOTHING fails, and nothing can: the periodic Hann window's first value is exactly 0 (test_window_table pins it),
     so fr[0] = v * 0 whatever v is -- the mutated kernel's output is bit-identical.  The fault it stands for, a scale dropped for one sample of a frame, was run as
 (b') ... for j == 200 (window value 1) instead: all nine test_pad_and_log_mel cases, all four test_batch_front_end cases, the log-mel checks of
     test_peak_is_found_wherever_it_lies[4097], [16385], [32769] (errors 3e-2 .. 3e-1), and test_stream_front_end_values (stream vs the single clip's front end).
 (c) absmax_kernel's tail loop starts one element later: test_peak_is_found_wherever_it_lies at all 15 lengths (the peak planted in the first tail element; at lengths
     that are a multiple of 4 the views at offsets 1 .. 3 have a tail), test_pad_and_log_mel[one_sample].
 (d) stream_mel_kernel `- 200 - left` -> `- 199 - left`: test_stream_front_end_values, test_stream_gain_reaches_the_mel (cut-independence holds, as it must: the
     shifted kernel is as deterministic as the right one).
 (e) stream_tick's first conv GEMM reads from halo + Cm (one frame late): test_stream_front_end_values (conv rows), test_stream_front_end_cut_independence.
No existing test failed under any of them in these runs (the id-level tests were not part of the runs; the issue's premise is that they would not notice)."""
import ctypes as C

import numpy as np
import pytest

import frontend_ref as F
from model_fixtures import tiny_gguf

pytestmark = pytest.mark.gpu
BAR = 1e-4


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield m
    m.close()


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.MelSpectrogram.mel_filterbank(), pkg.MelSpectrogram.hann_window(400)


class DevViews:
    """Device sample views `buf + off` (off in floats from a 256-byte aligned allocation): put(x, off) uploads x there and returns the pointer."""

    def __init__(self, pkg, ctx, floats):
        self.pkg, self.ctx, self.cap = pkg, ctx, floats
        self.base = ctx.alloc(4 * floats)
        assert self.base % 256 == 0

    def put(self, x, off):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert off >= 0 and off + x.size <= self.cap
        self.pkg._lib.check(self.pkg.lib().vox_dev_upload(self.ctx.h, C.c_void_p(self.base + 4 * off), x.ctypes.data_as(C.c_void_p), x.nbytes))
        return self.base + 4 * off

    def close(self):
        self.ctx.free(self.base)


_REF = {}


def ref_mel(key, x, scale, tables):
    """log_mel(pad(scale * x)) in float64, computed once per (clip, scale) and shared."""
    k = (key, float(scale))
    if k not in _REF:
        _REF[k] = F.log_mel(F.pad(np.float64(scale) * np.asarray(x, dtype=np.float64)), *tables)
        _REF[k].setflags(write=False)
    return _REF[k]


def check_mel(mel, key, x, scale, tables, noise=False):
    """Shape, layout, the bar, exact floor in the pad frames (and, for a noise clip, that the comparison is not floor against floor) -> worst |gpu - ref|."""
    ref = ref_mel(key, x, scale, tables)
    T = F.pad_len(len(x)) // 160
    assert ref.shape == (128, T) and mel.shape == (128, T) and mel.dtype == np.float32, (key, mel.shape, T)
    err = np.abs(mel - ref)
    assert np.isfinite(mel).all()
    worst = float(err.max())
    assert worst <= BAR, f"{key}: log-mel {worst:.3e} off the float64 reference at (mel bin, frame) {np.unravel_index(np.argmax(err), err.shape)}"
    inside = F.clip_frames(len(x), T)
    assert (mel[:, ~inside] == np.float32(F.FLOOR)).all(), f"{key}: a frame that sees only the pad is not at the floor exactly"
    if noise:
        assert (ref[:, inside] > F.FLOOR + 0.05).mean() >= 0.5, f"{key}: the clip's frames are mostly floor values"
    return worst


# ---- 1. peak reduction ------------------------------------------------------------------------------------------------------------------------------------------------
SWEEP = 4096      # float4 loads of one sweep of absmax_kernel (1024 threads x 4 in flight)
PEAK_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32769]
MEL_LENGTHS = {7, 4097, 16385, 32769}      # one length of each class also checks the log-mel


def plant_positions(n, off):
    """Where a peak can be lost, for samples whose pointer sits `off` floats past a 16-byte boundary: index 0, the last head element, the first and last element of the
    float4 body, both ends of float4 1023 / 1024 and 4095 / 4096 (the last of a thread's first batch / the first of its second; the last of a sweep / the first of the
    next), the first tail element, n - 1."""
    head = min(n, (4 - off) % 4); n4 = (n - head) // 4
    pos = {0, n - 1}
    if head:
        pos.add(head - 1)
    if n4:
        pos.update((head, head + 4 * n4 - 1))
    for q in (1023, 1024, SWEEP - 1, SWEEP):
        if q < n4:
            pos.update((head + 4 * q, head + 4 * q + 3))
    if head + 4 * n4 < n:
        pos.add(head + 4 * n4)
    return sorted(pos)


def background(n):
    rng = np.random.default_rng(n)
    return np.clip(0.1 * rng.standard_normal(n), -0.45, 0.45).astype(np.float32)


@pytest.mark.parametrize("n", PEAK_LENGTHS)
def test_peak_is_found_wherever_it_lies(pkg, ctx, model, tables, n):
    """Noise at 0.1 with one sample of +-0.7 planted in turn at every position plant_positions lists.  form 0 reads device views at every 16-byte phase; form 1 gets
    host units, which the driver packs back to back (units of 1, 2, 3 samples in between shift the phase from unit to unit).  The scale is exact in every case."""
    base = background(n)
    dv = DevViews(pkg, ctx, n + 8)
    try:
        cases = 0
        for off in range(4):
            for p in plant_positions(n, off):
                for sign in (1.0, -1.0):
                    x = base.copy(); x[p] = np.float32(sign * 0.7)
                    sc, mels = model.debug_front_end(None, 0, device_ptrs=[dv.put(x, off)], n_samples=[n])
                    assert sc[0] == F.peak_scale(x) == np.float32(0.95) / np.float32(0.7), (n, off, p, sign, sc[0])
                    cases += 1
        if n in MEL_LENGTHS:
            print(f"n {n}: form 0 log-mel of the last planted case {check_mel(mels[0], ('peak', n), x, sc[0], tables):.2e}")
    finally:
        dv.close()
    every = sorted(set().union(*[plant_positions(n, off) for off in range(4)]))
    units, planted = [], []
    for k, p in enumerate(every):
        for sign in (1.0, -1.0):
            x = base.copy(); x[p] = np.float32(sign * 0.7)
            planted.append(len(units)); units.append(x)
            units.append(np.full(1 + (len(units) // 2) % 3, 0.01, np.float32))      # 1, 2, 3 samples: moves the next unit's 16-byte phase
    for a in range(0, len(units), 126):
        sc, mels = model.debug_front_end(units[a:a + 126], 1)
        for j, x in enumerate(units[a:a + 126]):
            assert sc[j] == F.peak_scale(x), (n, a + j, sc[j])
    if n in MEL_LENGTHS:
        j = planted[-1] - a
        print(f"n {n}: form 1 log-mel of the last planted unit {check_mel(mels[j], ('peak', n), units[planted[-1]], sc[j], tables):.2e}")
    print(f"n {n}: {cases} form 0 cases, {len(planted)} form 1 units, every scale exact")


@pytest.mark.parametrize("mx,exp", [(0.0, 1.0), (9e-11, 1.0), (1e-10, None), (2e-10, None)])
def test_silence_threshold(pkg, ctx, model, mx, exp):
    """All-zero input and a maximum of 9e-11 give scale 1 exactly; 1e-10 and 2e-10 give 0.95 / max: single clip, batch unit, and group."""
    x = np.zeros(4099, np.float32); x[[0, 2049, 4098]] = np.float32(mx) * np.array([0.5, -1.0, 0.25], np.float32)
    want = np.float32(exp) if exp is not None else np.float32(0.95) / np.float32(mx)
    assert F.peak_scale(x) == want
    got = [model.debug_front_end([x], 0)[0][0], model.debug_front_end([x], 1)[0][0]] + list(model.debug_front_end([x, x[:17]], 1, norm_group=[3, 3])[0])
    assert all(g == want for g in got), (mx, got, want)


# ---- 2. pad and log-mel: single clip and batch ------------------------------------------------------------------------------------------------------------------------
def front_clips():
    edge = np.zeros(8000, np.float32); edge[0] = 0.7; edge[-1] = -0.7      # a pad boundary one sample off moves these across a frame's window
    c = {"0.1s": F.make_clip("noise", 1, 0.1), "one_sample": F.make_clip("one_sample"), "3s_noise": F.make_clip("noise", 2), "3s_tone_noise": F.make_clip("tone_noise", 3),
         "quiet_half": F.make_clip("quiet_half", 4), "edge_impulses": edge}
    for n in (3839, 3840, 3841):      # 97 280 + 3840 is a multiple of a token's 1280 samples: no round-up of the right pad, and one sample to either side of that
        c[f"n{n}"] = F.make_clip("noise", n, n / 16000)
        assert len(c[f"n{n}"]) == n
    return c


NOISE_CLIPS = {"0.1s", "3s_noise", "quiet_half", "n3839", "n3840", "n3841"}


@pytest.mark.parametrize("name", ["0.1s", "one_sample", "3s_noise", "3s_tone_noise", "quiet_half", "n3839", "n3840", "n3841", "edge_impulses"])
def test_pad_and_log_mel(pkg, ctx, model, tables, name):
    """The single clip's front end from host and from device memory and the batch front end on the same clip: T = pad_len / 160, layout [128][T], the pad's frames at
    the floor exactly, every value within the bar.  Whether the forms agree bit for bit is printed, not asserted."""
    x = front_clips()[name]; s = F.peak_scale(x); n = len(x)
    assert (F.LEFT + 3840) % F.SPT == 0 and F.pad_len(3840) + F.SPT == F.pad_len(3841) == F.pad_len(3839) + F.SPT
    dv = DevViews(pkg, ctx, n + 8)
    try:
        runs = {"form 0 host": model.debug_front_end([x], 0), "form 0 device": model.debug_front_end(None, 0, device_ptrs=[dv.put(x, 1)], n_samples=[n]),
                "form 1 host": model.debug_front_end([x], 1), "form 1 device": model.debug_front_end(None, 1, device_ptrs=[dv.put(x, 3)], n_samples=[n])}
    finally:
        dv.close()
    worst = {}
    for k, (sc, mels) in runs.items():
        assert sc[0] == s, (name, k, sc[0], s)
        worst[k] = check_mel(mels[0], name, x, s, tables, noise=name in NOISE_CLIPS)
    same = all(np.array_equal(runs["form 0 host"][1][0], r[1][0]) for r in runs.values())
    print(f"{name}: T {mels[0].shape[1]}, worst log-mel error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; forms bit-identical: {same}")


BATCH_LENGTHS = [1601, 4097, 799, 12345, 2561, 333, 7777]      # odd: the packed host units start at every 16-byte phase
BATCH_GROUPS = [5, 5, 5, 9, 9, 2, -1]      # three chunks of one file (its peak in the middle one), a silent file of two chunks, a file of one chunk, a unit used as it is


def batch_units():
    u = [F.make_clip("noise", 40 + i, n / 16000) for i, n in enumerate(BATCH_LENGTHS)]
    for i, peak in ((0, 0.3), (1, 0.9), (2, 0.5), (5, 0.6), (6, 0.2)):
        u[i] = (u[i] * np.float32(peak / np.abs(u[i]).max())).astype(np.float32)
    u[3][:] = 0; u[4][:] = 0
    assert [len(x) for x in u] == BATCH_LENGTHS
    return u


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("grouped", [False, True])
def test_batch_front_end(pkg, ctx, model, tables, mem, grouped):
    """Seven units of odd lengths through the batch front end, from host memory (packed by the driver) and as device views at odd offsets into one buffer; on their
    own peaks, and with the group mix of BATCH_GROUPS: every unit of a group gets the group's scale, a silent group and a unit with a negative group get 1."""
    u = batch_units(); grp = BATCH_GROUPS if grouped else None
    if grouped:
        want = []
        for i, g in enumerate(BATCH_GROUPS):
            want.append(np.float32(1.0) if g < 0 else F.peak_scale(np.concatenate([u[j] for j in range(7) if BATCH_GROUPS[j] == g])))
        assert want[0] == want[1] == want[2] == F.peak_scale(u[1]) and want[3] == want[4] == 1.0 and want[5] == F.peak_scale(u[5]) and want[6] == 1.0
    else:
        want = [F.peak_scale(x) for x in u]
        assert want[3] == 1.0 and len(set(float(w) for w in want)) == 6
    if mem == "host":
        sc, mels = model.debug_front_end(u, 1, norm_group=grp)
    else:
        dv = DevViews(pkg, ctx, sum(BATCH_LENGTHS) + 64)
        try:
            ptrs, o = [], 1
            for i, x in enumerate(u):
                ptrs.append(dv.put(x, o)); o += len(x) + (i % 3)      # offsets 1, 2, 0, 2, 1, ... floats past a 16-byte boundary
            assert {(p // 4) % 4 for p in ptrs} == {0, 1, 2, 3}
            sc, mels = model.debug_front_end(None, 1, norm_group=grp, device_ptrs=ptrs, n_samples=BATCH_LENGTHS)
        finally:
            dv.close()
    worst = 0.0
    for i, x in enumerate(u):
        assert sc[i] == want[i], (mem, grouped, i, sc[i], want[i])
        worst = max(worst, check_mel(mels[i], ("batch", i), x, want[i], tables, noise=i not in (3, 4)))
    print(f"batch front end, {mem} samples, {'grouped' if grouped else 'own peaks'}: scales exact, worst log-mel error {worst:.2e}")
