"""How many halvings a call that consumes full hit lists on the device makes, in plain Python.

The calls go through their queries in batches.  A batch's full lists go into hit buffers with room for `room` hits,
room = max((cluster_ws_mib << 20) // 16, N).  A batch (or a part of one) whose lists hold more than `room` hits is halved:
n queries become the first n // 2 and the other n - n // 2, the first half is finished before the second, and each half
is treated the same way.  Lists of exactly `room` hits fit.  One query cannot be halved: its list never holds more than
the N genomes, and room >= N.  The self-join calls (niqki_cluster, niqki_dereplicate, niqki_linkage) also shrink the
batches that follow a halved one to the smallest part of it that fitted; the query-side calls (niqki_query_collapsed,
niqki_query_lca) keep their batch size."""


def room(mib, n_genomes):
    return max((max(int(mib), 1) << 20) // 16, int(n_genomes))


def splits(lengths, batch, room, shrink):
    """lengths: the full list length of every query, in query order; batch: queries per batch; shrink: later batches
    take the size that fitted.  Returns the number of halvings."""
    lengths = [int(x) for x in lengths]
    count = 0

    def leaf(lo, n):
        """queries [lo, lo + n): the size of the smallest part that went through whole"""
        nonlocal count
        if sum(lengths[lo:lo + n]) <= room:
            return n
        if n == 1:
            raise ValueError("query %d alone has %d hits, the room is %d" % (lo, lengths[lo], room))
        count += 1
        h = n // 2
        first = leaf(lo, h)
        second = leaf(lo + h, n - h)
        return max(1, min(first, second))

    batch = max(int(batch), 1)
    at = 0
    while at < len(lengths):
        n = min(batch, len(lengths) - at)
        fitted = leaf(at, n)
        if shrink and fitted < n:
            batch = fitted
        at += n
    return count
