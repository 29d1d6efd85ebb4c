"""The OUTPUT CONTRACT of the device-resident entry points (include/fabgpu.h) on a context with FABGPU_FLAG_SHA3_COOP, in the manner of
tests/test_dev_output_contract_gpu.py and with its image helper: the digest rows lie in ONE guarded torch.uint8 allocation that is filled
with 0x00 and then with 0xFF, and after the call the whole allocation must equal the image built on the CPU - exactly n rows of
hashlib.sha3_256 digests and nothing in front of or behind them.  On the 32-lane prefixed road the caller's mid_scratch lies in the same
allocation and must read as filled ("n_prefixes x 200 bytes or nothing"); above SHA3_COOP_MAX a prefixed batch takes the one-lane road
and uses it.

Rows: 1, 2, 3 (one wavefront, half of it, one and a half), 65 (a partial last workgroup of eight rows), and SHA3_COOP_MAX + 1: the mixed
kernel for the plain batch, the one-lane kernel with mid-states for the prefixed one."""
import hashlib

import numpy as np
import pytest

import fabgpu
from dev_contract_image import ALIGN, FILLS, Layout, check

pytestmark = pytest.mark.gpu

SHA3_COOP_MAX = 4096                                  # csrc/kernels.h
ROWS = [1, 2, 3, 65, SHA3_COOP_MAX + 1]
NB = SHA3_COOP_MAX + 1
PRE = (300, 137)                                      # two shared prefixes; every third row has none


@pytest.fixture(scope="module")
def coop():
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_SHA3_COOP)
    yield c
    c.close()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


_base = {}


def base():
    """NB messages (a case of n rows is the first n), consecutive in one arena behind the two prefixes; their digests plain and prefixed"""
    if not _base:
        rng = np.random.default_rng(2049)
        lens = rng.integers(0, 300, size=NB)
        lens[:4] = (136, 0, 271, 135)
        lead = sum(PRE) + 5
        off = np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.uint32)
        arena = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
        pre_off = np.array([[2, 2 + PRE[0]], [3 + PRE[0], 3 + PRE[0] + PRE[1]]], dtype=np.uint32)
        pre_idx = np.array([0xFFFFFFFF if i % 3 == 2 else i % 3 for i in range(NB)], dtype=np.uint32)
        msgs = [arena[off[i]:off[i + 1]].tobytes() for i in range(NB)]
        pre = [arena[a:b].tobytes() for a, b in pre_off]
        dig = lambda ms: np.frombuffer(b"".join(hashlib.sha3_256(m).digest() for m in ms), dtype=np.uint8).reshape(-1, 32)
        one = np.zeros((NB, 32), np.uint8)
        one[:, 31] = 1
        _base.update(arena=arena, plain=dig(msgs), prefixed=dig([(pre[p] if p < 2 else b"") + m for p, m in zip(pre_idx, msgs)]),
                     dev=dict(arena=_up(arena), off=_up(off), spans=_up(np.stack([off[:-1], off[1:]], axis=1).astype(np.uint32)), pre_off=_up(pre_off),
                              pre_idx=_up(pre_idx), one=_up(one)))
    return _base


def run_both_fills(layout, call):
    import torch
    images = {}
    for fill in FILLS:
        buf = torch.full((layout.total,), fill, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % ALIGN == 0
        call({k: buf.data_ptr() + layout.offset[k] for k in layout.names})
        torch.cuda.synchronize()
        images[fill] = buf.cpu().numpy()
    return images


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("n", ROWS)
def test_hash_only_entry_writes_n_digest_rows_and_nothing_else(coop, n):
    """fabgpu_sha3_256_batch_dev: sha3_256_coop_kernel<false> up to SHA3_COOP_MAX rows, sha3_256_mixed_kernel above"""
    b = base()
    d = b["dev"]
    layout = Layout([("digests", 32 * n)])
    before = coop.sha3_coop_rows()
    images = run_both_fills(layout, lambda p: coop.sha3_256_batch_dev(n, d["arena"].data_ptr(), b["arena"].size, d["off"].data_ptr(), p["digests"], _stream()))
    lines = check(layout, images, dict(digests=b["plain"][:n]))
    assert not lines, "\n".join(lines)
    assert coop.sha3_coop_rows() - before == (2 * n if n <= SHA3_COOP_MAX else 0)     # (two runs; no message of the base is long)


@pytest.mark.parametrize("n", ROWS)
def test_described_batch_writes_n_digest_rows_and_leaves_mid_scratch_alone(coop, n):
    """fabgpu_identity_verify_batch_dev under FABGPU_IDB_SPANS | FABGPU_IDB_SHA3_256 with two prefixes: sha3_256_coop_kernel<true> up to
    SHA3_COOP_MAX rows - no mid-state launch, mid_scratch as filled -, sha3_256_midstate_kernel + sha3_256_batch_kernel<true> above, where
    mid_scratch is the call's to use.  (The verdict words and statuses of the meaningless signatures go to a buffer of their own.)"""
    import torch
    b = base()
    d = b["dev"]
    coop_road = n <= SHA3_COOP_MAX
    layout = Layout([("digests", 32 * n), ("mid_scratch", 2 * 200)])
    verdicts = torch.zeros((n + 63) // 64 * 8 + n, dtype=torch.uint8, device="cuda")

    def call(p):
        q = fabgpu._IdBatch()
        q.n, q.flags = n, fabgpu.IDB_SPANS | fabgpu.IDB_SHA3_256
        q.arena, q.arena_bytes, q.off = d["arena"].data_ptr(), b["arena"].size, d["spans"].data_ptr()
        q.n_prefixes, q.pre_off, q.pre_idx = 2, d["pre_off"].data_ptr(), d["pre_idx"].data_ptr()
        q.qx = q.qy = q.r = q.s = d["one"].data_ptr()
        q.verdict_bits, q.status, q.digests = verdicts.data_ptr(), verdicts.data_ptr() + (n + 63) // 64 * 8, p["digests"]
        coop.identity_verify_batch_dev(q, p["mid_scratch"], _stream())

    lines = check(layout, run_both_fills(layout, call), dict(digests=b["prefixed"][:n]), scratch=() if coop_road else ("mid_scratch",))
    assert not lines, "\n".join(lines)
