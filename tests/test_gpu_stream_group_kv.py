"""Paged stream groups with a bf16 K/V pool (vox_stream_group_create_kv, VOX_KV_BF16) end to end on the tiny models and at full size: pool() and pages() equal the f32
paged group's after every call, only bf16 attention forms launch, logits within 4x the measured gap and ids by the group files' rule, layer-0 rows exactly the rounded
f32 rows, snapshot / reset / restore bit for bit (also behind an endless group's table wrap), reset and reuse, a refused call, a peek, the records.  The tests and their
reasoning are tests/stream_group_kv_worker.py's; they run there through pytest in a process of their own, because a bf16 group's decode attention counts in
vox_debug_attn_launches [16] .. [19], which other tests of the suite hold to 0 in their process.  Each test here asserts that its case passed there; the worker's
output (the measured gaps among it) is printed."""
import pytest

from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
CASES = ["test_bf16_group_against_the_f32_paged_group[head]", "test_bf16_group_against_the_f32_paged_group[gqa]",
         "test_layer0_rows_are_the_rounded_rows_of_the_f32_member[head]", "test_layer0_rows_are_the_rounded_rows_of_the_f32_member[gqa]",
         "test_snapshot_reset_restore_of_a_bf16_member_continues_bit_for_bit[head]", "test_snapshot_reset_restore_of_a_bf16_member_continues_bit_for_bit[gqa]",
         "test_endless_bf16_member_resumes_behind_the_table_wrap", "test_reset_and_reuse_leave_nothing_behind", "test_a_refused_call_leaves_pool_and_tables_untouched",
         "test_a_peek_leaves_the_group_what_it_was", "test_scores_and_alternatives_are_functions_of_the_tapped_row",
         "test_full_size_three_members_against_the_f32_paged_group"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = run_worker("stream_group_kv_worker.py", tmp_path_factory.mktemp("group_kv"), 900)
    print(r[1][-4000:])
    return r


@pytest.mark.parametrize("name", CASES)
def test_worker_case(run, name):
    check(run, name)


def test_every_case_of_the_worker_is_asserted_here(run):
    assert set(run[0]) == set(CASES), sorted(set(run[0]) ^ set(CASES))
