"""The two index maps of the persistent kernels' schedulers (csrc/dsdf_lane.h), checked on the host build: exact integer properties.

tail_hop(first, k): the k-th tail sub-queue a persistent consumer visits when it starts at `first` (sub-queue = XCD * 8 + ticket counter).
Every sub-queue must be drained whatever XCD a block lands on, and a block should empty the queues of its own XCD first.

item_of(share, j): the j-th work item of one of the 8 shares of the work list (segment s of DSDF_ITEM_SEG items belongs to share s % 8).
The ticket walk of the work-list workers relies on two things: the shares partition the list, and the items of a share ascend -- so a
share is exhausted at its first item >= n_items."""
import pytest


def test_tail_hop_is_a_permutation_that_starts_in_its_own_xcd(harness):
    hop = harness.lib.hh_tail_hop
    for first in range(64):
        order = [hop(first, k) for k in range(64)]
        assert sorted(order) == list(range(64)), f"first={first}: not a permutation of the 64 sub-queues"
        assert order[0] == first
        assert all(q >> 3 == first >> 3 for q in order[:8]), f"first={first}: the first 8 hops leave its XCD: {order[:8]}"
        # ... and then one XCD after the other, 8 queues each
        for x in range(8):
            assert len({q >> 3 for q in order[8 * x:8 * x + 8]}) == 1


def test_item_of_partitions_the_work_list_and_ascends_within_a_share(harness):
    item_of, seg = harness.lib.hh_item_of, harness.lib.hh_item_seg()
    assert seg > 0
    for n_items in (0, 1, 7, seg - 1, seg, seg + 1, 3 * seg + 5, 8 * seg, 8 * seg + 1, 19 * seg + seg // 2, 40 * seg - 1):
        seen = []
        for share in range(8):
            prev, j = -1, 0
            while True:
                it = item_of(share, j)
                assert it > prev, f"share {share}: item_of does not ascend at j={j}"
                if it >= n_items:           # the walk's test: the share is exhausted
                    break
                seen.append(it)
                prev, j = it, j + 1
            # nothing below n_items follows the first item at or beyond it (spot-check one segment further)
            assert all(item_of(share, j + d) >= n_items for d in range(1, seg + 2, max(1, seg // 7)))
        assert sorted(seen) == list(range(n_items)), f"n_items={n_items}: the 8 shares do not hand out every item exactly once"
