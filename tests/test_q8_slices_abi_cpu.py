"""The Q8_0 K-slice operator's public symbols without a GPU: exported by the library, declared in the header, bound in the ctypes layer; null arguments are refused."""
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxtral_hip.h")


@pytest.mark.parametrize("name", ["vox_q8_rows_forward", "vox_q8_rows_launches"])
def test_symbol_is_exported_declared_and_bound(pkg, name):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert hasattr(pkg.lib(), name) and re.search(r"\b%s\s*\(" % name, hdr) and name in pkg._lib.SIGNATURES


def test_null_arguments_are_refused(pkg):
    L = pkg.lib()
    assert L.vox_q8_rows_forward(None, None, None, None, 0.0, None, 1, None, 0, 0, None, 0) == 1 and b"null argument" in L.vox_last_error() and L.vox_q8_rows_launches(None) == 1
    assert callable(pkg.q8_rows_forward) and callable(pkg.q8_rows_launches)
