"""The decode engine's paired MFMA steps (vox_engine.hip: mstep2 -- two K-steps per epilogue, lane groups 0, 1 finish one step and groups 2, 3 the other, every
per-lane operand chosen by lane group) against the per-operator launches, on the smallest model the engine accepts: the real decoder geometry (the engine requires
it) with TWO decoder layers and one encoder layer.  Two layers cover a layer-to-layer hand-over, both all-gather buffers and w2's odd step count (four pairs and a
single step, one pair spanning two tiles).  One model has N(0, sigma) weights, the other heavy_tail=True: Student-t block scales and outlier channels, where a block
scale or a block info taken from the wrong lane group's step is orders of magnitude off instead of a little.  2 s clip; the bound is the full-size test's (2e-4 of the
largest |logit| on every step, equal ids); the engine is run-to-run bit-identical and its graph-replayed ids equal its eager ids."""
import os

import numpy as np
import pytest

from model_fixtures import cache_dir

pytestmark = pytest.mark.gpu
TOL = 2e-4


@pytest.fixture(scope="module", params=[(52, False), (53, True)], ids=["normal", "heavy_tail"])
def small(pkg, request):
    seed, heavy = request.param
    S = pkg.synth
    path = os.path.join(cache_dir(), f"dec2_enc1_q4_seed{seed}{'_heavytail' if heavy else ''}.gguf")
    if not os.path.exists(path):
        S.write_synthetic_gguf(path + f".tmp{os.getpid()}", S.ModelDims(dec_layers=2, enc_layers=1), seed=seed, heavy_tail=heavy); os.replace(path + f".tmp{os.getpid()}", path)
    ctx = pkg.Context(0)
    m = pkg.Q4ModelLoader.from_file(path).load(ctx)
    x = S.synth_audio(2.0, seed=97)
    mel = np.ascontiguousarray(pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(pkg.peak_normalize(x))).T)[None]
    yield m, mel, pkg.TimeEmbedding(3072).embed(6.0)
    m.close(); ctx.close()


def test_paired_steps_engine_vs_per_operator_path(small):
    m, mel, t = small
    if not m.set_decode_engine(True):
        pytest.skip("decode engine not available on this device (needs 256 CUs)")
    ids_e, lg_e = m.transcribe_streaming(mel, t, return_logits=True)
    ids_e2, lg_e2 = m.transcribe_streaming(mel, t, return_logits=True)
    ids_g = m.transcribe_streaming(mel, t)                                  # graph replay
    assert not m.set_decode_engine(False)
    ids_o, lg_o = m.transcribe_streaming(mel, t, return_logits=True)
    m.set_decode_engine(True)
    assert len(ids_e) == len(ids_o) and len(ids_e) >= 8
    err = np.abs(lg_e - lg_o).max(axis=1); top = float(np.abs(lg_o).max())
    print(f"paired steps, 2-layer decoder ({len(ids_e)} ids): max |dlogit| {float(err.max()):.3e} at step {int(err.argmax())} (largest |logit| {top:.2f}), "
          f"ids equal: {np.array_equal(ids_e, ids_o)}")
    assert np.array_equal(ids_e, ids_o)
    assert (err <= TOL * top).all()                                         # on every step
    assert np.array_equal(ids_e, ids_e2) and np.array_equal(lg_e, lg_e2)    # run-to-run bit-identical
    assert np.array_equal(ids_g, ids_e)                                     # graph-replayed ids == eager ids
