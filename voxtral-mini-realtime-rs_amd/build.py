"""Builds libvoxtral_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.environ.get("VOX_LIB") or os.path.join(PKG_DIR, "libvoxtral_hip.so")   # VOX_LIB: a measurement build (variant_lib_path)
# host units ("Host units"): the device-free ones include no HIP header and are compiled as plain C++
HOST_SOURCES_PLAIN = ["vox_audio_host.cpp", "vox_gguf.cpp", "vox_batch_plan.cpp", "vox_feed_plan.cpp", "vox_snapshot_plan.cpp"]
HOST_SOURCES = ["vox_api.cpp", "vox_model.cpp", "vox_ctx.cpp", "vox_tensor.cpp", "vox_cache.cpp", *HOST_SOURCES_PLAIN]
SOURCES = ["vox_kernels.hip", "vox_engine.hip", "vox_engine_b16.hip", *HOST_SOURCES]
HEADERS = ["vox_kernels.h", "vox_engine_common.h", "vox_page_pool.h", "vox_kv_bf16.h", "vox_snapshot.h", "vox_host_base.h", "vox_dev_base.h", os.path.join("..", "..", "include", "voxtral_hip.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def variant_lib_path(tag: str) -> str:
    return os.path.join(PKG_DIR, f"libvoxtral_hip_{tag}.so")


def build_all(verbose: bool = False, force: bool = False, tag: str | None = None, extra_flags=()) -> str:
    """Product build (tag None): build/*.o -> libvoxtral_hip.so.  Measurement variants (`tag`, e.g. "timeline" with
    extra_flags=["-DVOX_TIMELINE"]): build/<tag>/*.o -> libvoxtral_hip_<tag>.so, selected at run time with VOX_LIB=<that path>."""
    bdir = os.path.join(PKG_DIR, "build", tag) if tag else os.path.join(PKG_DIR, "build")
    lib_path = variant_lib_path(tag) if tag else LIB_PATH
    os.makedirs(bdir, exist_ok=True)
    deps = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(bdir, src.rsplit(".", 1)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [sp] + deps):
            jobs.append([HIPCC, *FLAGS, *extra_flags, "-x", "c++" if src in HOST_SOURCES_PLAIN else "hip", "-c", sp, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), 16))) as ex:
        list(ex.map(run, jobs))
    if jobs or force or _stale(lib_path, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_path, *objs])
    return lib_path


VARIANTS = {"timeline": ["-DVOX_TIMELINE"]}      # measurement build (tools/timeline.py)

if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:
        print(build_all(verbose=True, tag=sys.argv[1], extra_flags=VARIANTS.get(sys.argv[1], sys.argv[2:])))
    else:
        print(build_all(verbose=True))
