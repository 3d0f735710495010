"""The fused tick's public symbols without a GPU: exported by the library, declared in the header, bound in the ctypes layer; null arguments are refused."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxtral_hip.h")


@pytest.mark.parametrize("name", ["vox_stream_set_tick_fused", "vox_stream_tick_fused", "vox_debug_rows4_op", "vox_debug_rows4_launches"])
def test_symbol_is_exported_declared_and_bound(pkg, name):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert hasattr(pkg.lib(), name) and re.search(r"\b%s\s*\(" % name, hdr) and name in pkg._lib.SIGNATURES


def test_null_arguments_are_refused(pkg):
    L = pkg.lib(); assert L.vox_stream_set_tick_fused(None, 1) == 1 and b"null stream" in L.vox_last_error() and L.vox_stream_tick_fused(None) == 0
    assert L.vox_debug_rows4_op(None, None, None, None, 0.0, None, 1, None, 0, 0, None) == 1 and L.vox_debug_rows4_launches(None) == 1
