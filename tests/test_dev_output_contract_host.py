"""The checker of tests/test_dev_output_contract_gpu.py against hand-made images (numpy only): it passes the image a correct _dev call
leaves, and names every defect the GPU test exists to find - a byte in a guard, a verdict bit at n, a part of a verdict word nobody
wrote (the three widths the kernels own words by: a byte, 16 bits, 32 bits), a status byte and a digest row at row n."""
import numpy as np
import pytest

from dev_contract_image import FILLS, GUARD, Layout, check, compare, expected_image, verdict_words

N = 70                                                     # two verdict words, six rows in the last


def _case():
    rng = np.random.default_rng(70)
    status = rng.integers(0, 4, size=N).astype(np.uint8)
    status[64], status[65] = 0, 1                          # both answers in the last word
    digests = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    layout = Layout([("verdict_bits", (N + 63) // 64 * 8), ("status", N), ("digests", 32 * N)])
    return layout, dict(verdict_bits=verdict_words(status == 0), status=status, digests=digests)


def _correct(layout, written):
    return {fill: expected_image(layout, fill, written) for fill in FILLS}


def test_layout_aligns_and_guards_every_region():
    layout, _ = _case()
    ends = 0
    for name in layout.names:
        assert layout.offset[name] % 256 == 0 and layout.offset[name] - ends >= GUARD
        ends = layout.offset[name] + layout.size[name]
    assert layout.total - ends >= GUARD
    assert layout.where(layout.offset["status"] + N) == ("status", N) and layout.where(3) == ("verdict_bits", 3 - layout.offset["verdict_bits"])


def test_verdict_words_are_little_endian_with_zeros_from_n_on():
    v = np.zeros(N, dtype=bool)
    v[[0, 9, 63, 64, 69]] = True
    w = verdict_words(v).view("<u8")
    assert w.tolist() == [1 | 1 << 9 | 1 << 63, 1 | 1 << 5]
    assert verdict_words(np.ones(64, dtype=bool)).view("<u8").tolist() == [2**64 - 1] and verdict_words(np.ones(1, dtype=bool)).size == 8


def test_a_correct_image_passes():
    layout, written = _case()
    assert check(layout, _correct(layout, written), written) == []
    without = {k: v for k, v in written.items() if k != "status"}          # status == NULL: the region stays as filled
    assert check(layout, _correct(layout, without), without) == []
    assert check(layout, _correct(layout, written), without) != []         # ... and a call that writes it all the same is caught


@pytest.mark.parametrize("where", ["front", "behind"])
def test_a_flipped_guard_byte_is_reported(where):
    layout, written = _case()
    images = _correct(layout, written)
    pos = layout.offset["verdict_bits"] - 1 if where == "front" else layout.offset["digests"] + 32 * N + GUARD - 1
    for fill in FILLS:
        images[fill][pos] ^= 0x01
    lines = check(layout, images, written)
    assert len(lines) == 2
    if where == "front":
        assert "in front of region verdict_bits, offset -1: got 0x01 want 0x00" in lines[0] and lines[1].startswith("fill 0xff")
    else:
        assert "behind region digests, offset +%d: got 0xfe want 0xff" % (32 * N + GUARD - 1) in lines[1]


def test_a_set_bit_at_n_is_reported():
    layout, written = _case()
    images = _correct(layout, written)
    for fill in FILLS:
        images[fill][layout.offset["verdict_bits"] + 8] |= 1 << (N - 64)   # bit 6 of the last word
    lines = check(layout, images, written)
    want = int(written["verdict_bits"][8])
    assert want & 0xC3 == 0x01                                               # rows 64 (valid) and 65 (not), nothing from bit 6 on
    assert len(lines) == 2 and all("in region verdict_bits, offset +8: got 0x%02x want 0x%02x" % (want | 0x40, want) in x for x in lines)


@pytest.mark.parametrize("width,at", [(1, 9), (2, 10), (4, 12)], ids=["byte", "16 bits", "32 bits"])
def test_an_unwritten_part_of_the_last_word_shows_under_one_fill_only(width, at):
    """what a kernel leaves behind that forgets the tail of the last word (the eight-lane form's zeroing loop, the fused four-lane form
    with i0 < n for its guard, the two-lane form's upper half): the part keeps the fill - and zero is what it should hold"""
    layout, written = _case()
    images = _correct(layout, written)
    o = layout.offset["verdict_bits"] + at
    for fill in FILLS:
        images[fill][o:o + width] = fill
    assert compare(layout, images[0x00], expected_image(layout, 0x00, written)) == []
    lines = check(layout, images, written)
    assert len(lines) == width and all(x.startswith("fill 0xff: in region verdict_bits, offset +") and "got 0xff want 0x00" in x for x in lines)
    assert "offset %+d:" % at in lines[0]


def test_an_unwritten_part_that_should_hold_ones_shows_under_the_other_fill():
    layout, written = _case()
    written["verdict_bits"] = verdict_words(np.ones(N, dtype=bool))
    images = _correct(layout, written)
    o = layout.offset["verdict_bits"] + 2
    for fill in FILLS:
        images[fill][o:o + 2] = fill
    lines = check(layout, images, written)
    assert len(lines) == 2 and all(x.startswith("fill 0x00: in region verdict_bits") and "got 0x00 want 0xff" in x for x in lines)


def test_a_status_byte_at_row_n_is_reported():
    layout, written = _case()
    images = _correct(layout, written)
    for fill in FILLS:
        images[fill][layout.offset["status"] + N] = 1
    lines = check(layout, images, written)
    assert len(lines) == 2 and "behind region status, offset +%d: got 0x01 want 0x00" % N in lines[0]


def test_a_digest_row_at_row_n_is_reported():
    layout, written = _case()
    images = _correct(layout, written)
    row = np.arange(32, dtype=np.uint8) + 1
    for fill in FILLS:
        images[fill][layout.offset["digests"] + 32 * N:layout.offset["digests"] + 32 * N + 32] = row
    lines = check(layout, images, written)
    assert sum("behind region digests, offset +%d:" % (32 * N + k) in x for x in lines for k in range(32)) >= 24   # (the report stops at 12 bytes a run)
    assert "offset +%d: got 0x01 want 0x00" % (32 * N) in lines[0]


def test_a_scratch_region_is_free_inside_and_guarded_outside():
    layout = Layout([("mid_scratch", 64), ("status", 3)])
    written = dict(status=np.array([0, 1, 2], dtype=np.uint8))
    images = _correct(layout, written)
    for fill in FILLS:
        images[fill][layout.offset["mid_scratch"]:layout.offset["mid_scratch"] + 64] = 0x5A
    assert check(layout, images, written, scratch=("mid_scratch",)) == [] and check(layout, images, written) != []
    images[0x00][layout.offset["mid_scratch"] + 64] = 0x5A
    assert check(layout, images, written, scratch=("mid_scratch",)) == ["fill 0x00: behind region mid_scratch, offset +64: got 0x5a want 0x00"]
