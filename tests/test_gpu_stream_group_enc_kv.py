"""Stream groups with a bf16 encoder K/V ring (vox_stream_group_create_enc_kv, VOX_KV_BF16) end to end on the tiny model.  The tests and their reasoning are
tests/stream_group_enc_kv_worker.py's; they run there through pytest in a process of their own, because one of the group kinds has a bf16 K/V pool, whose decode
attention counts in vox_debug_attn_launches [16] .. [19], which other tests of the suite hold to 0 in their process.  Each test here asserts that its case passed
there; the worker's output (the measured gaps among it) is printed."""
import pytest

from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
CASES = [f"test_bf16_ring_group_against_the_f32_ring_group[{k}]" for k in ("slab", "paged", "endless", "bf16pool", "burst")] + \
        [f"test_ids_and_logits_do_not_depend_on_the_cut[{k}]" for k in ("slab", "paged")] + [f"test_a_peek_leaves_every_later_id_and_logit[{k}]" for k in ("slab", "burst")] + \
        [f"test_snapshot_reset_restore_continues_bit_for_bit[{k}]" for k in ("slab", "endless")] + ["test_f32_by_the_new_creator_is_the_existing_group"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = run_worker("stream_group_enc_kv_worker.py", tmp_path_factory.mktemp("group_enc_kv"), 600)
    print(r[1][-4000:])
    return r


@pytest.mark.parametrize("name", CASES)
def test_worker_case(run, name):
    check(run, name)


def test_every_case_of_the_worker_is_asserted_here(run):
    assert set(run[0]) == set(CASES), sorted(set(run[0]) ^ set(CASES))
