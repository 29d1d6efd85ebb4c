"""The image side of tests/test_dev_output_contract_gpu.py (numpy only: no GPU, no library): where the output regions of a _dev call lie
in one allocation, what the whole allocation must hold after the call, and the byte-for-byte comparison that names what differs.

The contract (include/fabgpu.h, "OUTPUT CONTRACT of the _dev entry points"): every verdict word fully written with zeros at and above
bit n, status[0, n), digests[0, n) - and not one byte more.  A call is run twice, over an allocation filled with 0x00 and with 0xFF:
a byte the call leaves unwritten differs from the expected image in one of the two runs at least, a byte it writes where it should
not shows in the other."""
import numpy as np

GUARD = 256                    # bytes nobody may touch in front of the first region, behind the last and between any two
ALIGN = 256                    # every region starts on a multiple of it (the API wants 16)
FILLS = (0x00, 0xFF)


class Layout:
    """regions: [(name, owned bytes)] in the order they lie.  offset[name] is a multiple of ALIGN; at least GUARD bytes that belong to
    nobody lie in front of every region and behind the last."""

    def __init__(self, regions):
        self.names, self.offset, self.size = [], {}, {}
        pos = 0
        for name, size in regions:
            assert name not in self.offset and size >= 0
            pos = (pos + GUARD + ALIGN - 1) // ALIGN * ALIGN
            self.names.append(name)
            self.offset[name], self.size[name] = pos, int(size)
            pos += int(size)
        self.total = (pos + GUARD + ALIGN - 1) // ALIGN * ALIGN

    def where(self, pos):
        """(region, offset relative to it) of a byte of the allocation: the region that starts at or before it - an offset at or beyond
        the region's size is a byte BEHIND it -, for the bytes in front of the first region that one, with a negative offset"""
        name = self.names[0]
        for k in self.names:
            if self.offset[k] <= pos:
                name = k
        return name, pos - self.offset[name]


def verdict_words(valid):
    """bool[n] -> the bytes of ceil(n / 64) little-endian u64 words: bit i % 64 of word i / 64 set where row i is valid, zeros from n on"""
    valid = np.asarray(valid, dtype=bool)
    bits = np.zeros((valid.size + 63) // 64 * 64, dtype=np.uint8)
    bits[:valid.size] = valid
    return np.packbits(bits, bitorder="little")


def expected_image(layout, fill, written):
    """the whole allocation as it must read after the call: `fill` everywhere but in written[name] (uint8 arrays, at most the region's
    size), which lie at the start of their regions.  A region that is not in `written` stays as filled."""
    img = np.full(layout.total, fill, dtype=np.uint8)
    for name, data in written.items():
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert data.size <= layout.size[name], (name, data.size, layout.size[name])
        img[layout.offset[name]:layout.offset[name] + data.size] = data
    return img


def compare(layout, got, want, scratch=(), limit=12):
    """-> one line per differing byte (the first `limit` of them; empty: the images are equal): region, offset relative to the region,
    got / want.  scratch: regions whose own bytes are the call's to use as it likes - only the bytes around them are compared."""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    assert got.shape == want.shape == (layout.total,)
    differs = got != want
    for name in scratch:
        differs[layout.offset[name]:layout.offset[name] + layout.size[name]] = False
    out = []
    bad = np.nonzero(differs)[0]
    for pos in bad[:limit]:
        name, rel = layout.where(int(pos))
        side = "in front of" if rel < 0 else ("behind" if rel >= layout.size[name] else "in")
        out.append("%s region %s, offset %+d: got 0x%02x want 0x%02x" % (side, name, rel, got[pos], want[pos]))
    if bad.size > limit:
        out.append("... and %d more bytes" % (bad.size - limit))
    return out


def check(layout, images, written, scratch=()):
    """images: {fill: the allocation as read back after the run over that fill}, one per FILLS -> the differences of both runs, each
    line led by its fill"""
    assert sorted(images) == sorted(FILLS)
    out = []
    for fill in FILLS:
        out += ["fill 0x%02x: %s" % (fill, line) for line in compare(layout, images[fill], expected_image(layout, fill, written), scratch)]
    return out
