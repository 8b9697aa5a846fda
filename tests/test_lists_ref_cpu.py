"""CPU: tests/lists_ref.py, the halvings of a call that consumes full hit lists, on length vectors whose answers are
counted by hand in the comments.  The GPU suites compare the calls' *_splits counters with this function."""
import pytest

from lists_ref import room, splits


def test_room_is_a_sixteenth_of_the_budget_and_never_below_the_genome_count():
    assert room(1, 3000) == 65536
    assert room(1024, 3000) == 1 << 26
    assert room(1, 70000) == 70000
    assert room(0, 10) == 65536                      # the option is taken as at least 1 MiB


@pytest.mark.parametrize("shrink", [False, True])
def test_hand_counted_cases(shrink):
    # no split: 3 + 4 + 2 + 1 = 10 hits in a room of 10
    assert splits([3, 4, 2, 1], 4, 10, shrink) == 0
    # nothing to do
    assert splits([], 4, 10, shrink) == 0
    # one split at the top: 14 > 10; [5, 5] = 10 fits, [2, 2] fits
    assert splits([5, 5, 2, 2], 4, 10, shrink) == 1
    # a split in the second half only: 17 > 10 (1); [1, 1] fits; [8, 7] = 15 > 10 (2); [8] and [7] fit
    assert splits([1, 1, 8, 7], 4, 10, shrink) == 2
    # an odd batch: 5 queries become 2 + 3; 25 > 10 (1); [5, 5] fits; [5, 5, 5] > 10 (2); [5] fits, [5, 5] fits
    assert splits([5, 5, 5, 5, 5], 5, 10, shrink) == 2
    # a batch of one query that fits exactly: the total equals the room
    assert splits([10], 1, 10, shrink) == 0
    assert splits([10, 10, 10], 1, 10, shrink) == 0
    # every level splits: 40 > 10 (1), both halves 20 > 10 (2, 3), the four single queries fit
    assert splits([10, 10, 10, 10], 4, 10, shrink) == 3


def test_the_shrink_carries_over_to_the_next_batch():
    lengths = [6, 6, 1, 1, 6, 6, 1, 1]
    # batches of 4 in a room of 10.  Batch 1: 14 > 10 (1); [6, 6] > 10 (2); [6], [6] fit; [1, 1] fits: the smallest
    # part that fitted holds 1 query.
    # Without the shrink batch 2 is the same four queries again: 2 more.
    assert splits(lengths, 4, 10, False) == 4
    # With it the four remaining queries go one at a time and each fits.
    assert splits(lengths, 4, 10, True) == 2
    # The size that fitted is the smaller of the halves' sizes: batch 1 = [6, 6, 1, 1 | ...] of 8 queries, 28 > 10 (1);
    # first half [6, 6, 1, 1] as above (2, 3), fitted 1; second half the same (4, 5).  One batch, nothing to carry.
    assert splits(lengths, 8, 10, True) == 5 == splits(lengths, 8, 10, False)
    # the batch size never grows back: [9, 9] splits once, then every query goes alone although [1, 1, 1, 1] would fit
    assert splits([9, 9, 1, 1, 1, 1], 2, 10, True) == 1
    assert splits([9, 9, 9, 9, 1, 1], 2, 10, False) == 2
    assert splits([9, 9, 9, 9, 1, 1], 2, 10, True) == 1


def test_one_query_above_the_room_cannot_be_halved():
    with pytest.raises(ValueError):
        splits([11], 1, 10, False)
    with pytest.raises(ValueError):
        splits([1, 11], 2, 10, True)
