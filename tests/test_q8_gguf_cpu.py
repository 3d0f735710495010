"""Q8_0 in the GGUF reader (GGML type 8: 34 bytes per 32 elements) and gguf.quantize_q8_0; no device."""
import numpy as np
import pytest


def _image(pkg, tmp_path, code):
    S = pkg.synth; rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, 16 * 2 * (34 if code == S.GGML_Q8_0 else 18), dtype=np.uint8); f = rng.standard_normal(24).astype(np.float32)
    p = str(tmp_path / f"t{code}.gguf")
    S.write_gguf(p, [("w.q8", (16, 64), code, raw), ("v.f32", (24,), S.GGML_F32, f)])
    return open(p, "rb").read(), raw, f


def test_reader_takes_q8_0(pkg, tmp_path):
    img, raw, f = _image(pkg, tmp_path, 8)
    r = pkg.GgufReader.from_bytes(img)
    info = r.tensor_info("w.q8")
    assert (info.dtype(), info.shape(), info.byte_size()) == (8, [64, 16], 16 * 2 * 34)
    assert (r.tensor_data("w.q8") == raw).all() and (r.tensor_data("v.f32").view(np.float32) == f).all()
    r.close()


def test_reader_still_refuses_type_7(pkg, tmp_path):
    with pytest.raises(pkg.VoxError, match="Unsupported GGML dtype code: 7"):
        pkg.GgufReader.from_bytes(_image(pkg, tmp_path, 7)[0])


def test_quantize_q8_0_blocks(pkg):
    rng = np.random.default_rng(9)
    x = np.stack([np.zeros(32), np.where(np.arange(32) == 5, -3.0, 0.4 * rng.standard_normal(32).clip(-2, 2)), rng.standard_normal(32)]).astype(np.float32)
    b = pkg.quantize_q8_0(x).reshape(3, 34)
    d = np.ascontiguousarray(b[:, :2]).view(np.float16).reshape(3); q = b[:, 2:].view(np.int8).astype(np.float32)
    assert (d == (np.abs(x).max(axis=1) / np.float32(127)).astype(np.float16)).all() and d[0] == 0 and (q[0] == 0).all() and q[1, 5] == -127
    df = d.astype(np.float32)[:, None]
    assert (q[1:] == np.rint(x[1:] / df[1:])).all() and (np.abs(df * q - x) <= 0.5 * df * (1 + 2.0 ** -20)).all()
