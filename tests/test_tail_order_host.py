"""The order of a workgroup's range in the fused 3x3 kernel and the walk its epilogue makes over an item's segments,
restated in Python next to fused_work_layout() and sk_start() (csrc/wino_f2_fused_kernel.h) and checked over every small
launch shape.  No GPU needed.

The rule: a workgroup whose tail range lies inside ONE tail item (one tail segment) runs its whole-item rounds first and
that segment last ("whole-first"); every other workgroup runs its tail first.  The whole-first workgroup is then its tail
item's natural last arriver: when it peeks at the item's counter, the other segments have usually drawn long ago, and it
finishes the item from its registers.  Nothing rests on that being so -- a peek that finds less takes the ticket path --
but the cut must be what the kernel believes it is: the segments of an item, found by the epilogue's walk outwards from
the workgroup's own range, must be exactly the ranges that hold chunks of the item, in order, each chunk once."""
import pytest

BC, KB = 8, 64


def sk_start(l, q, rem, G):
    return l * q + l * rem // G


def fused_work_layout(C, K, items, G):
    """ndp, sk_q, sk_rem, kp, Gp as the host computes them."""
    nchunks, kblk = C // BC, K // KB
    kp = 1 if kblk <= 1 or G % kblk != 0 else kblk
    Tg, Gp = (items % G) * nchunks // kp, G // kp
    return items // G, Tg // Gp, Tg % Gp, kp, Gp


def tail_range(lp, q, rem, Gp):
    return sk_start(lp, q, rem, Gp), sk_start(lp + 1, q, rem, Gp)


def whole_first(ndp, nchunks, t_begin, Lt):
    """The kernel's prologue: t_chunk + Lt <= nchunks."""
    return ndp > 0 and Lt > 0 and t_begin % nchunks + Lt <= nchunks


def order_of_range(ndp, nchunks, t_begin, Lt):
    """The segments a workgroup computes, in its order: ('whole', round) and ('tail', item-in-group, first, count)."""
    tail, t = [], t_begin
    while t < t_begin + Lt:
        n = min(t_begin + Lt - t, nchunks - t % nchunks)
        tail.append(("tail", t // nchunks, t % nchunks, n))
        t += n
    rounds = [("whole", r) for r in range(ndp)]
    return rounds + tail if whole_first(ndp, nchunks, t_begin, Lt) else tail + rounds


def epilogue_walk(lp, item, nchunks, q, rem, Gp):
    """The epilogue's walk outwards from range lp over the ranges that share tail item `item` of its k-group:
    (gA, gB, nseg), empty ranges not counted."""
    x0, x1 = item * nchunks, item * nchunks + nchunks - 1
    gA = gB = lp
    while sk_start(gA, q, rem, Gp) > x0:
        gA -= 1
    while gB + 1 < Gp and sk_start(gB + 1, q, rem, Gp) <= x1:
        gB += 1
    nseg = sum(sk_start(g + 1, q, rem, Gp) != sk_start(g, q, rem, Gp) for g in range(gA, gB + 1))
    return gA, gB, nseg


SHAPES = [(C, items, G) for C in (64, 128, 256) for items in range(1, 65) for G in range(1, 49)]


@pytest.mark.parametrize("C", [64, 128, 256])
def test_order_rule_and_segment_walk(C):
    nchunks = C // BC
    seen_whole_first = seen_straddler = seen_unequal = seen_kp = 0
    for C_, items, G in SHAPES:
        if C_ != C:
            continue
        # items come K/64 per tile block: take every K/64 that divides the item count, as the launch would have it
        for kblk in (1, 2, 4):
            if items % kblk:
                continue
            ndp, q, rem, kp, Gp = fused_work_layout(C, kblk * KB, items, G)
            tail_items = (items % G) // kp             # per k-group
            assert (items % G) % kp == 0
            assert q * Gp + rem == tail_items * nchunks
            seen_unequal += rem != 0
            seen_kp += kp > 1
            cover = [[0] * nchunks for _ in range(tail_items)]
            segs = [[] for _ in range(tail_items)]       # per item: (range, first chunk, count), in range order
            arrivers = [[] for _ in range(tail_items)]   # per item: the whole-first ranges that end in it
            for lp in range(Gp):
                a, b = tail_range(lp, q, rem, Gp)
                order = order_of_range(ndp, nchunks, a, b - a)
                tails = [s for s in order if s[0] == "tail"]
                # every iteration of the range exactly once, whatever the order
                assert sum(s[3] for s in tails) == b - a and sum(s[0] == "whole" for s in order) == ndp
                # (3) the whole-first rule selects exactly the ranges with one tail segment (where there are rounds
                # to run first; without rounds the two orders are the same)
                wf = whole_first(ndp, nchunks, a, b - a)
                assert wf == (ndp > 0 and len(tails) == 1), (C, items, G, lp)
                if wf:
                    assert order[-1][0] == "tail" and [s[0] for s in order[:-1]] == ["whole"] * ndp
                    arrivers[tails[0][1]].append(lp)
                    seen_whole_first += 1
                elif tails:
                    assert order[0][0] == "tail"
                    seen_straddler += len(tails) > 1
                for _, item, first, n in tails:
                    for c in range(first, first + n):
                        cover[item][c] += 1
                    segs[item].append((lp, first, n))
            for item in range(tail_items):
                # (1) every item's segments cover its chunks exactly once, in range order
                assert cover[item] == [1] * nchunks, (C, items, G, item)
                assert [s[1] for s in segs[item]] == sorted(s[1] for s in segs[item])
                owners = [s[0] for s in segs[item]]
                for lp in owners:   # ... and the kernel's walk, from any of them, finds exactly those ranges
                    gA, gB, nseg = epilogue_walk(lp, item, nchunks, q, rem, Gp)
                    assert (gA, gB, nseg) == (owners[0], owners[-1], len(owners)), (C, items, G, item, lp)
                    if q > 0:   # the gather from registers relies on it: no empty range between gA and gB
                        assert gB - gA + 1 == nseg
                # (2) each item has exactly one designated natural last arriver or none.  The whole-first ranges that
                # end in an item are its one-segment ranges; the designated one is the LAST of them in segment order --
                # a rule that names one for every shape, also where ranges shorter than half an item put several
                # one-segment ranges inside one item.  (All of those peek, and the counter lets at most one wave per
                # part through: a peek only succeeds once every OTHER segment has drawn, and a peeking segment draws
                # only after its own peek has failed.  Whoever it is, the sum keeps its segment order.)
                if ndp > 0:
                    inside = [lp for lp, first, n in segs[item] if tail_range(lp, q, rem, Gp) == (item * nchunks + first, item * nchunks + first + n)]
                    assert arrivers[item] == inside
                    designated = [lp for lp in inside if lp == max(inside)]
                    assert len(designated) == (1 if inside else 0), (C, items, G, item)
                    if designated:
                        d = designated[0]
                        assert d in owners and whole_first(ndp, nchunks, *(lambda a, b: (a, b - a))(*tail_range(d, q, rem, Gp)))
                        # every other segment of the item belongs to a straddler (tail first: published at least one
                        # whole item before the designated range gets there) or to an earlier one-segment range
                        for lp in owners:
                            assert lp == d or lp not in inside or lp < d
                    if 2 * q > nchunks:   # ranges longer than half an item: no second one-segment range fits
                        assert len(inside) <= 1, (C, items, G, item)
                else:
                    assert arrivers[item] == []   # no rounds to run first: nobody is whole-first
    assert seen_whole_first and seen_straddler and seen_unequal and seen_kp


def test_headline_cut():
    """256 channels, N = 128: 392 items on 256 workgroups, kp = 4, 64 ranges of 17 over 34 items of 32 per k-group."""
    ndp, q, rem, kp, Gp = fused_work_layout(256, 256, 392, 256)
    assert (ndp, q, rem, kp, Gp) == (1, 17, 0, 4, 64)
    wf = [whole_first(ndp, 32, *(lambda a, b: (a, b - a))(*tail_range(lp, q, rem, Gp))) for lp in range(Gp)]
    assert sum(wf) == 32   # half of the ranges start in the first 16 chunks of an item: 128 of the 256 workgroups
    nsegs = [epilogue_walk((item * 32) // 17, item, 32, q, rem, Gp)[2] for item in range(34)]
    assert sorted(set(nsegs)) == [2, 3] and nsegs.count(2) == 6
