"""bench.py without a GPU: the in-memory synthetic GGUF it loads, and the model file it writes for the tools."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("vox_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed,threads,enc_bias", [(42, 1, True), (42, 4, True), (7, 3, False)])
def test_bench_gguf_image_is_the_synth_file(pkg, tmp_path, seed, threads, enc_bias):
    """The image bench.py builds in memory is byte for byte the file synth.write_synthetic_gguf writes, whatever the thread count."""
    S = pkg.synth
    dims = S.tiny_dims(enc_bias=enc_bias)
    path = str(tmp_path / "m.gguf")
    S.write_synthetic_gguf(path, dims, seed=seed)
    ref = np.fromfile(path, dtype=np.uint8)
    img = _bench().synthetic_gguf_image(S, dims, seed, threads=threads)
    assert img.dtype == np.uint8 and img.size == ref.size
    assert np.array_equal(img, ref)


def test_bench_gguf_header_only_image(pkg, tmp_path):
    """Ranks > 0 get the same header and size with zero tensor data, and the library parses both images to the same tensor table."""
    S = pkg.synth
    dims = S.tiny_dims()
    b = _bench()
    full = b.synthetic_gguf_image(S, dims, 42, threads=2)
    head = b.synthetic_gguf_image(S, dims, 42, header_only=True)
    assert head.size == full.size
    r_full, r_head = pkg.GgufReader.from_bytes(full), pkg.GgufReader.from_bytes(head)
    try:
        names = r_full.tensor_names()
        assert names == r_head.tensor_names() and len(names) == len(S.tensor_manifest(dims))
        for n in names:
            a, h = r_full.tensor_info(n), r_head.tensor_info(n)
            assert (a.shape(), a.dtype(), a.byte_size()) == (h.shape(), h.dtype(), h.byte_size())
            assert not r_head.tensor_data(n).any()
    finally:
        r_full.close(); r_head.close()
    k = int(np.flatnonzero(full != head)[0])      # the header ends before the first weight byte
    assert np.array_equal(full[:k], head[:k]) and not head[k:].any()


def test_tools_use_only_what_bench_defines():
    """The measurement scripts under tools/ that `import bench` call only names bench.py still defines."""
    import re
    b = _bench()
    tools = os.path.join(ROOT, "tools")
    used = {}
    for f in sorted(os.listdir(tools)):
        if f.endswith(".py"):
            src = open(os.path.join(tools, f)).read()
            if re.search(r"^import bench\b", src, re.M):
                for name in set(re.findall(r"\bbench\.(\w+)", src)) - {"py"}:      # (not "bench.py" in a docstring)
                    used.setdefault(name, []).append(f)
    assert used, "no tool imports bench"
    missing = {n: fs for n, fs in used.items() if not hasattr(b, n)}
    assert not missing, missing


def test_bench_gguf_file_is_the_golden_model(pkg, tmp_path, monkeypatch):
    """At full size the model file bench.full_gguf_path writes for the tools, built by the in-memory builder, is the model the committed 16 s oracle
    golden was made on (the same SHA-256 as its GGUF file); a second call reuses it."""
    import hashlib
    g = np.load(os.path.join(ROOT, "tests", "golden", "fullsize_16s_oracle.npz"))
    monkeypatch.setenv("VOX_BENCH_DIR", str(tmp_path))
    b = _bench()
    path = b.full_gguf_path(pkg, 42, 0, lambda: None)
    assert os.path.dirname(path) == str(tmp_path) and os.listdir(str(tmp_path)) == [os.path.basename(path)]
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    assert h.digest() == g["gguf_sha256"].tobytes()
    mtime = os.path.getmtime(path)
    assert b.full_gguf_path(pkg, 42, 0, lambda: None) == path and os.path.getmtime(path) == mtime
