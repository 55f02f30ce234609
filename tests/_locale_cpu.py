"""Host restatement of the locale guide's contract (include/bgnn_locale.h): ``locale_guide`` writes it out in Python integers, cell by
cell, with float64 only for the one rounding; ``locale_guide_np`` is the same in numpy for the larger planes, a sort along the
window axis with a sentinel for what is no witness, in chunks of rows.  Both return ``guide`` as uint32 bits and ``support`` as
int32.  The device tests compare with them bit for bit; test_host_locale.py holds them against each other and brute force."""
import numpy as np

MAX_RADIUS = 8
NAN_BITS = 0x7FC00000
VALUE_TOP = 2 ** 32 - 1                                  # |center2| of a witness stays below 2^32


def guide_bits(med2):
    """``(float)((double)med2 * 2^-18)`` as uint32 bits: the product is exact in float64, the cast rounds once."""
    return int(np.float32(np.float64(med2) * np.float64(2.0 ** -18)).view(np.uint32))


def check_args(shape, radius, min_support):
    assert len(shape) == 2 and shape[0] >= 1 and shape[1] >= 1 and shape[0] * shape[1] <= 2 ** 31 - 1
    assert 1 <= radius <= MAX_RADIUS and 1 <= min_support <= (2 * radius + 1) ** 2 - 1


def locale_guide(n_hyp, chosen, center2, radius, min_support):
    """``(guide_bits, support)`` in the planes' shape, in Python integers."""
    n_hyp, chosen, center2 = np.asarray(n_hyp), np.asarray(chosen), np.asarray(center2)
    height, width = n_hyp.shape
    check_args(n_hyp.shape, radius, min_support)
    witness = [[int(n_hyp[r, c]) == 1 and int(chosen[r, c]) == 0 for c in range(width)] for r in range(height)]
    value = [[int(center2[r, c]) for c in range(width)] for r in range(height)]
    guide = np.full((height, width), NAN_BITS, np.uint32)
    support = np.zeros((height, width), np.int32)
    for r in range(height):
        for c in range(width):
            w = sorted(value[rr][cc]
                       for rr in range(max(r - radius, 0), min(r + radius, height - 1) + 1)
                       for cc in range(max(c - radius, 0), min(c + radius, width - 1) + 1)
                       if (rr, cc) != (r, c) and witness[rr][cc])
            k = len(w)
            support[r, c] = k
            if k >= min_support:
                guide[r, c] = guide_bits(w[(k - 1) // 2] + w[k // 2])
    return guide, support


def locale_guide_np(n_hyp, chosen, center2, radius, min_support, chunk_rows=64):
    """The same from a sentinel sort along the window axis, ``chunk_rows`` rows of the plane at a time."""
    n_hyp, chosen, center2 = np.asarray(n_hyp), np.asarray(chosen), np.asarray(center2, np.int64)
    height, width = n_hyp.shape
    check_args(n_hyp.shape, radius, min_support)
    sentinel = np.int64(2 ** 61)                                                     # above every value; two of them still add up
    padded = np.full((height + 2 * radius, width + 2 * radius), sentinel, np.int64)
    padded[radius:radius + height, radius:radius + width] = np.where((n_hyp == 1) & (chosen == 0), center2, sentinel)
    offsets = [(dr, dc) for dr in range(2 * radius + 1) for dc in range(2 * radius + 1) if (dr, dc) != (radius, radius)]
    guide = np.full((height, width), NAN_BITS, np.uint32)
    support = np.zeros((height, width), np.int32)
    for lo in range(0, height, chunk_rows):
        hi = min(lo + chunk_rows, height)
        stack = np.stack([padded[lo + dr:hi + dr, dc:dc + width] for dr, dc in offsets], axis=-1)
        stack.sort(axis=-1)
        k = (stack != sentinel).sum(axis=-1)
        support[lo:hi] = k
        safe = np.maximum(k, 1)
        a = np.take_along_axis(stack, ((safe - 1) // 2)[..., None], axis=-1)[..., 0]
        b = np.take_along_axis(stack, (safe // 2)[..., None], axis=-1)[..., 0]
        bits = ((a + b).astype(np.float64) * np.float64(2.0 ** -18)).astype(np.float32).view(np.uint32)      # (exact below 2^53)
        guide[lo:hi] = np.where(k >= min_support, bits, np.uint32(NAN_BITS))
    return guide, support


def random_planes(rng, shape, share, spread):
    """``n_hyp``, ``chosen``, ``center2`` with about ``share`` of the cells witnesses and the rest every way of being none (empty,
    two hypotheses, one that was not chosen); the values of all cells, witnesses or not, uniform in ``-spread .. spread``."""
    kind = rng.integers(0, 3, shape)
    is_w = rng.random(shape) < share
    n_hyp = np.where(is_w, 1, np.array([0, 2, 1])[kind]).astype(np.int32)
    chosen = np.where(is_w, 0, np.array([-1, 0, -1])[kind]).astype(np.int32)
    center2 = rng.integers(-spread, spread + 1, shape).astype(np.int64)
    return n_hyp, chosen, center2
