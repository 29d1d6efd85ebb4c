"""The scalar sets that more than one test walks u1 G + u2 Q with: the adversarial (u1, u2) of the combined multiplication and the
u2 at the edges of the window recoding.  Kept in one place so that the host test, the whole-signature test and the device-primitive
tests cannot drift apart."""
import bccsp_sw_oracle as po

N = po.N


def adversarial_u2s(rng):
    """Digits at every edge of the 5-bit Booth windows (0, 1, 25, 50, 51), long carry runs, n - small; then 40 random ones."""
    u2s = [1, 2, 15, 16, 17, 31, 32, 33, (1 << 255), (1 << 256) % N, N - 1, N - 2, N - 16, N - 17, N >> 1, (1 << 250) - 1,
           int("5" * 64, 16) % N, int("a" * 63, 16), int("f" * 63, 16), int("84210" * 12, 16) % N, int("7bdef" * 12, 16) % N]
    for w in (0, 1, 25, 50, 51):
        for d in range(1, 32):
            v = (d << (5 * w)) % N
            if v:
                u2s.append(v)
    return u2s + [rng.randrange(1, N) for _ in range(40)]


def adversarial_u1s(rng):
    """Comb-window corners of u1 (16-bit windows), then 8 random ones.  Call it after adversarial_u2s with the same rng."""
    return [0, 1, 255, 256, 65535, 65536, (1 << 240), (1 << 248), N - 1, int("ff00" * 16, 16) % N, int("ffff0000" * 8, 16) % N,
            int("0001" * 16, 16)] + [rng.randrange(N) for _ in range(8)]


def edge_u2_targets():
    """u2 = n - 2 (the scalar whose product the main wave takes from the table) and the other recoding edges."""
    return [N - 2, N - 1, N - 3, N - 16, N - 17, N - 18, N - 32, N - 34, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33,
            (1 << 255) - 1, 1 << 255, (1 << 255) + 8, (1 << 256) % N, int("8" * 64, 16) % N, int("7" * 64, 16), int("f" * 63, 16),
            int("1" * 64, 16), N >> 1, (N >> 1) + 1]
