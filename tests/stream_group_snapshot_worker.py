"""Worker of tests/test_gpu_stream_group_snapshot.py: the endless paged group's same-slot case runs through pytest in a process of its own (worker_tests.run_worker) --
an endless group launches the paged attention on ring page tables, whose launch counts (vox_debug_attn_launches [14] [15]) the suite's other tests hold to 0 in their
own process.  Not collected by the suite (no test_ prefix)."""
import pytest

from model_fixtures import tiny_gguf
from snapshot_group_cases import same_slot_case

pytestmark = pytest.mark.gpu


def test_endless_member_snapshot_reset_restore_in_its_slot(pkg):
    ctx = pkg.Context(0)
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    try:
        same_slot_case(pkg, m, "endless")
    finally:
        m.close(); ctx.close()
