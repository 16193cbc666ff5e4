"""The signal-batch convention on the host: the prefix sums, the key-major offsets and the flattening of
nested offset lists that sepkern/ops.py and sepkern/data.py state once, against plain loops written out here.  No GPU."""
import pytest

from sepkern import _lib, ops
from sepkern.data import key_offsets


def test_prefix_sums():
    assert ops.prefix_sums([5]) == ([0], 5)
    assert ops.prefix_sums([3, 1, 4]) == ([0, 3, 4], 8)
    assert ops.prefix_sums([]) == ([], 0)
    assert ops._lengths("w", [5], 1) == ([5], [0], 5)
    assert ops._lengths("w", (3, 1, 4), 1) == ([3, 1, 4], [0, 3, 4], 8)
    assert ops._lengths("w", [3, 0, 4], 0) == ([3, 0, 4], [0, 3, 3], 7)
    assert ops._lengths("w", [3, -1], None) == ([3, -1], [0, 3], 2)               # no minimum: the C side refuses
    for ns, least in (([], 1), ([], None), ([3, 0, 4], 1), ([3, -1], 0)):
        with pytest.raises(_lib.SepkernError, match="^w needs"):
            ops._lengths("w", ns, least)


def test_key_major_offsets():
    assert key_offsets([5], [0]) == [[0]]
    assert key_offsets([3, 1, 4], [0]) == [[0, 3, 4]]
    assert key_offsets([3, 1, 4], range(3)) == [[0, 3, 4], [8, 11, 12], [16, 19, 20]]
    assert key_offsets([3, 1, 4], [0, 3, 2]) == [[0, 3, 4], [24, 27, 28], [16, 19, 20]]       # the keys a caller picks, in its order
    assert key_offsets([], [0, 1]) == [[], []]


def test_offset_lists_are_flattened_in_the_order_the_kernels_read_them():
    ns = [3, 1, 4]
    B, S, P, numel = 3, 2, 3, 100
    src, chan = (1, 4, "source"), (1, 7, "channel")
    one = [10, 20, 30]
    two = [[10 * s + b for b in range(B)] for s in range(S)]
    three = [[[30 * s + 10 * p + b for b in range(B)] for p in range(P)] for s in range(S)]
    assert ops._offsets("w", one, ns, numel) == ([one[b] for b in range(B)],)
    assert ops._offsets("w", two, ns, numel, src) == ([two[s][b] for s in range(S) for b in range(B)], S)
    assert ops._offsets("w", three, ns, numel, src, chan) == ([three[s][p][b] for s in range(S) for p in range(P) for b in range(B)], S, P)
    # any iterables, as the wrappers took them: the counts come from what was read, not from len() of the argument
    assert ops._offsets("w", (tuple(r) for r in two), ns, numel, (2, 2, "source")) == ([o for r in two for o in r], 2)
    # the signal that ends with the buffer is taken, one sample further is not; every leaf is checked against ITS length
    assert ops._offsets("w", [[97, 99, 96]], ns, numel, (1, 1, "source")) == ([97, 99, 96], 1)
    for bad in ([[98, 99, 96]], [[97, 100, 96]], [[97, 99, 97]], [[-1, 0, 0]]):
        with pytest.raises(_lib.SepkernError, match="^w: a signal runs past its buffer"):
            ops._offsets("w", bad, ns, numel, (1, 1, "source"))
    with pytest.raises(_lib.SepkernError, match="^w: a signal runs past"):
        ops._offsets("w", [0, 0], [3, -1], numel)                                           # a negative length, in the same pass
    # the number of lists at every level, named in the message, and one offset per utterance in every innermost list
    with pytest.raises(_lib.SepkernError, match=r"^w needs 3\.\.4 lists of offsets, one per source, .* \(got 2\)"):
        ops._offsets("w", two, ns, numel, (3, 4, "source"))
    for bad, counts in ((two, ((1, 1, "source"),)), (three, (src, (1, 2, "channel"))), ([two[0], two[1][:2]], (src,)),
                        ([three[0], three[1][:2]], (src, chan)), (one[:2], ()), ([], (src,))):
        with pytest.raises(_lib.SepkernError, match="^w needs"):
            ops._offsets("w", bad, ns, numel, *counts)
