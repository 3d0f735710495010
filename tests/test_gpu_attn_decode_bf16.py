"""The paged decode attention on a bf16 K/V pool (AttnParams::kv_bf16; vox_debug_attn_decode_paged_bf16), one launch at a time: bf16 pool == f32 pool of the widened
values bit for bit, both forms, flat and ring tables, rows and XF planes out; the float64 reference at the bar of tests/test_gpu_attn_decode.py; the launch counters.
The tests and their reasoning are tests/attn_decode_bf16_worker.py's; they run there through pytest in a process of their own, because the reference launches on ring
tables count in vox_debug_attn_launches [14] [15] and the bf16 launches in [16] .. [19], which other tests of the suite hold to 0 in their process.  Each test here
asserts that its case passed there."""
import pytest

from attn_decode_bf16_worker import CASES as WORKER_CASES
from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
CASES = [f"test_bf16_attention_is_the_f32_attention_on_the_widened_values[{kind}-{name}-{out}]" for out in ("rows", "xf") for name in WORKER_CASES for kind in ("head", "gqa")] + \
        ["test_refusals_launch_nothing"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = run_worker("attn_decode_bf16_worker.py", tmp_path_factory.mktemp("attn_bf16"), 600)
    print(r[1][-3000:])
    return r


@pytest.mark.parametrize("name", CASES)
def test_worker_case(run, name):
    check(run, name)


def test_every_case_of_the_worker_is_asserted_here(run):
    assert set(run[0]) == set(CASES), sorted(set(run[0]) ^ set(CASES))
