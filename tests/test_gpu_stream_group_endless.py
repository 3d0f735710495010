"""Endless paged stream groups (vox_stream_group_create_endless) end to end on the tiny models: endless == bounded paged bit for bit with three interleaving members
(both attention forms), across the window and the page table's wrap (also with a changed entry range that wraps), two members past 16 384 positions, and the CLI.  The tests and their reasoning are
tests/stream_group_endless_worker.py's; they run there through pytest in a process of their own, because an endless group's decode attention counts in
vox_debug_attn_launches [14] [15], which other tests of the suite hold to 0 in their process.  Each test here asserts that its case passed there; the worker's output
(the seconds of the long runs among it) is printed."""
import pytest

from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
CASES = ["test_endless_group_equals_the_bounded_paged_group_bit_for_bit[head-14-11]", "test_endless_group_equals_the_bounded_paged_group_bit_for_bit[gqa-15-12]",
         "test_past_the_window_and_across_the_table_wrap", "test_a_call_that_enters_two_pages_across_the_table_wrap_and_a_reset_of_a_wrapped_range",
         "test_two_members_past_16384_positions", "test_cli_live_group_endless_prints_the_paged_group_lines"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = run_worker("stream_group_endless_worker.py", tmp_path_factory.mktemp("group_endless"), 900)
    print(r[1][-3000:])
    return r


@pytest.mark.parametrize("name", CASES)
def test_worker_case(run, name):
    check(run, name)


def test_every_case_of_the_worker_is_asserted_here(run):
    assert set(run[0]) == set(CASES), sorted(set(run[0]) ^ set(CASES))
