"""Scalars for the all-odd 4-bit recoding of u2 in the LDS-table pair kernels (csrc/p256_odd4.h), shared by the host test of the recoding
and the device test of the kernels.  A target is a value of u2; the recoding folds it to the odd one of u2 and n - u2, k, and reads
h = k >> 1 in 64 four-bit windows."""
import bccsp_sw_oracle as po

N = po.N


def _k_of_h(nibbles_top_first):
    h = 0
    for x in nibbles_top_first:
        h = h << 4 | x
    return 2 * h + 1


def named_u2():
    """Small and large u2, the halves of n and the powers of two around bit 255: every one below n."""
    return [1, 2, 3, 4, 15, 16, 17, N - 1, N - 2, N - 3, N - 4, N - 15, N - 16, N - 17, (N - 1) // 2, (N + 1) // 2,
            1 << 255, (1 << 255) - 1, (1 << 255) + 1]


def window_patterns():
    """k whose 64 windows h_i are all 0, all 7, all 8, all 15, alternating 7 / 8 (both phases), under a top window of 0 (top digit 1)
    and of 7 (top digit 15).  Those at or above n (all 15 under a top window of 7 is 2^256 - 1) are for the host test alone."""
    out = []
    for top in (0, 7):
        for body in ([0] * 63, [7] * 63, [8] * 63, [15] * 63, [7, 8] * 31 + [7], [8, 7] * 31 + [8]):
            out.append(_k_of_h([top] + body))
    out.append(_k_of_h([7] * 64))
    return out


def device_u2():
    """Every target a signature can carry (0 < u2 < n): the named ones, and each window pattern below n both as u2 = k and as
    u2 = n - k (the fold's two sides)."""
    t = list(named_u2())
    for k in window_patterns():
        if k < N:
            t += [k, N - k]
    seen, out = set(), []
    for u in t:
        if 0 < u < N and u not in seen:
            seen.add(u)
            out.append(u)
    return out


def recode(u2):
    """The recoding in Python integers: (k, sign, digits), digits[i] = d_i of k (the fold's sign NOT applied), window 0 first."""
    sign = 0 if u2 & 1 else 1
    k = N - u2 if sign else u2
    h = k >> 1
    hs = [(h >> (4 * i)) & 15 for i in range(64)]
    return k, sign, [2 * x - 15 for x in hs[:63]] + [2 * hs[63] + 1]


def exceptional_windows(digits):
    """Windows i at which the chain's addition meets M == +-d (mod n): T = M Q before the addition, addend d Q."""
    bad = []
    M = digits[63]
    for i in range(62, -1, -1):
        M *= 16
        if (M - digits[i]) % N == 0 or (M + digits[i]) % N == 0:
            bad.append(i)
        M += digits[i]
    return bad
