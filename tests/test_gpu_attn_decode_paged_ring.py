"""The paged decode attention on a RING page table (AttnParams::page_tab_len; vox_debug_attn_decode_paged_ring), one launch at a time: ring table == flat table bit
for bit, in both forms, at L = 19 and 32, positions to 2^24 - 1; the counter slots; the refusals.  The cases and their reasoning are tests/attn_paged_ring_worker.py's;
they run there through pytest in a process of their own, because ring-table launches count in vox_debug_attn_launches [14] [15], which other tests of the suite hold to
0 in their process.  Each test here asserts that its case passed there; the worker's output is printed."""
import pytest

from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
CASES = [f"test_ring_table_equals_flat_table_bit_for_bit[{kind}-{L}]" for L in (19, 32) for kind in ("head", "gqa")] + [
    "test_a_wider_stride_than_the_ring_is_read_by_the_ring_length", "test_refusals_launch_nothing"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = run_worker("attn_paged_ring_worker.py", tmp_path_factory.mktemp("attn_paged_ring"), 300)
    print(r[1][-2000:])
    return r


@pytest.mark.parametrize("name", CASES)
def test_worker_case(run, name):
    check(run, name)


def test_every_case_of_the_worker_is_asserted_here(run):
    assert set(run[0]) == set(CASES), sorted(set(run[0]) ^ set(CASES))
