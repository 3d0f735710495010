"""The bf16 encoder ring's entry points are exported by the built library and declared for ctypes (no GPU: the symbols are looked up, nothing is called)."""
import ctypes

NAMES = ("vox_stream_group_create_enc_kv", "vox_stream_group_enc_kv_dtype", "vox_debug_stream_attn_elem")


def test_enc_kv_symbols_are_exported_and_declared(pkg):
    L = ctypes.CDLL(pkg.build.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in pkg._lib.SIGNATURES, f"{name} has no ctypes signature"
    assert len(pkg._lib.SIGNATURES["vox_stream_group_create_enc_kv"][1]) == len(pkg._lib.SIGNATURES["vox_stream_group_create_t_embeds"][1]) + 1
