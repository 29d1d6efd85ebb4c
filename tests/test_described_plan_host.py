"""DescribedPlan (csrc/described_plan.h), the span plan of a described batch, on the CPU: the one place where a caller's offsets become
device offsets, driven through the stand-alone program csrc/hosttest_described_plan.cpp (descriptions on stdin, one answer line each;
the sanitizer build of the same program is `make sanitize-described-plan`).  The model below is written from the contract of
fabgpu_identity_batch in include/fabgpu.h, not from the C++: the refusal code, lo, hi, tail_used, the gather total and every rebased
offset of every description must agree."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_described_plan")
EINVAL, ETOOBIG = -1, -5
MAX_END, MAX_GATHER = 0xFFFFFFF0, 0x7FFFFFF0


def D(place="own", spans=True, prefix_in_tail=False, tail=None, off=(), pre=(), nym=(), gather=()):
    """A description.  tail: (tail_base, tail_len) or None; off / pre: pairs with spans, else consecutive offsets; nym: pairs; gather:
    rows of three pairs."""
    return dict(place=place, spans=spans, prefix_in_tail=prefix_in_tail, tail=tail, off=list(off), pre=list(pre), nym=list(nym), gather=list(gather))


def model(d):
    """What include/fabgpu.h says of a description: ("refused", code) or ("ok", lo, hi, tail_used, gather_total, [rebased arrays])."""
    spans, tail = d["spans"], d["tail"]
    base, tlen = tail if tail else (None, 0)
    bad = False
    if tail and (base % 64 or not spans or base + tlen > MAX_END):
        bad = True                                         # a tail: in spans mode only, at a multiple of 64, within the 32-bit offsets
    used, tail_used = [], False                            # the non-empty arena spans; whether anything addresses the tail

    def pair(s0, s1, may_be_tail):
        nonlocal bad, tail_used
        if s1 < s0:
            bad = True
        elif s1 > s0:
            if base is not None and s0 >= base:            # offsets >= tail_base address tail[offset - tail_base]
                tail_used = True
                if not may_be_tail or s1 > base + tlen:
                    bad = True
            elif base is not None and s1 > base:           # a span may not straddle tail_base
                bad = True
            else:
                used.append((s0, s1))

    def rows(o, may_be_tail):
        nonlocal bad
        if spans:
            for i in range(0, len(o), 2):
                pair(o[i], o[i + 1], may_be_tail)
        elif any(b < a for a, b in zip(o, o[1:])):
            bad = True
        elif len(o) > 1:
            used.append((o[0], o[-1]))                     # consecutive messages: everything from the first offset to the last, empty ends included

    rows(d["off"], True)
    for i in range(0, len(d["nym"]), 2):
        pair(d["nym"][i], d["nym"][i + 1], True)
    rows(d["pre"], d["prefix_in_tail"])
    total = 0
    for i in range(0, len(d["gather"]), 2):                # gathered pieces come from the caller's arena only
        s0, s1 = d["gather"][i], d["gather"][i + 1]
        if s1 < s0 or (s1 > s0 and base is not None and s1 > base):
            bad = True
        elif s1 > s0:
            used.append((s0, s1))
            total += s1 - s0
    if bad:
        return ("refused", EINVAL)
    if total > MAX_GATHER:
        return ("refused", ETOOBIG)
    lo = min((u[0] for u in used), default=0)
    hi = max((u[1] for u in used), default=0)
    if tail_used and d["place"] == "arena":
        lo = 0                                             # the tail lies in the device arena AT tail_base: nothing moves

    def rebased(o, pairs):
        if not pairs:
            return [v - lo for v in o]
        out = []
        for i in range(0, len(o), 2):
            s0, s1 = o[i], o[i + 1]
            by = 0 if base is not None and s0 >= base else lo
            out += [s0 - by, s1 - by] if s1 > s0 else [0, 0]
        return out

    return ("ok", lo, hi, int(tail_used), total, [rebased(d["off"], spans), rebased(d["pre"], spans), rebased(d["nym"], True), rebased(d["gather"], True)])


def line(d):
    spans = d["spans"]
    n = len(d["off"]) // 2 if spans else len(d["off"]) - 1
    m = len(d["pre"]) // 2 if spans else max(len(d["pre"]) - 1, 0)
    base, tlen = d["tail"] if d["tail"] else (0, 0)
    head = [d["place"], int(spans), int(d["prefix_in_tail"]), int(d["tail"] is not None), base, tlen, n, m, len(d["nym"]) // 2, len(d["gather"]) // 6]
    return " ".join(str(x) for x in head + d["off"] + d["pre"] + d["nym"] + d["gather"])


def answers(ds):
    out = subprocess.run([EXE], input="\n".join(line(d) for d in ds) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = []
    for text in out.stdout.splitlines():
        w = text.split("|")
        head = w[0].split()
        if head[0] == "refused":
            got.append(("refused", int(head[1])))
        else:
            got.append(("ok", int(head[1]), int(head[2]), int(head[3]), int(head[4]), [[int(v) for v in part.split()] for part in w[1:]]))
    assert len(got) == len(ds)
    return got


T = (1024, 100)                                            # a tail of 100 bytes at 1024
G = 1 << 31
CRAFTED = {
    "empty span": (D(off=[7, 7, 10, 20]), ("ok", 10, 20, 0, 0)),
    "reversed span": (D(off=[10, 20, 9, 8]), EINVAL),
    "span ending exactly at tail_base": (D(tail=T, off=[1000, 1024, 1024, 1030]), ("ok", 1000, 1024, 1, 0)),
    "span starting exactly at tail_base": (D(tail=T, off=[1024, 1025]), ("ok", 0, 0, 1, 0)),
    "span straddling by one byte": (D(tail=T, off=[1000, 1025]), EINVAL),
    "tail span ending at the tail's end": (D(tail=T, off=[1100, 1124]), ("ok", 0, 0, 1, 0)),
    "tail span ending one byte past the tail's end": (D(tail=T, off=[1100, 1125]), EINVAL),
    "prefix in the tail, refused": (D(tail=T, off=[0, 5], pre=[1024, 1030]), EINVAL),
    "prefix in the tail, permitted": (D(tail=T, off=[0, 5], pre=[1024, 1030], prefix_in_tail=True), ("ok", 0, 5, 1, 0)),
    "consecutive offsets with empty first and last messages": (D(spans=False, off=[40, 40, 50, 60, 60], pre=[30, 30, 35]), ("ok", 30, 60, 0, 0)),
    "consecutive offsets with a decrease": (D(spans=False, off=[40, 50, 49]), EINVAL),
    "nothing referencing the arena": (D(tail=T, off=[5, 5, 1024, 1030], pre=[9, 9]), ("ok", 0, 0, 1, 0)),
    "tail_base not a multiple of 64": (D(tail=(1000, 100), off=[0, 5]), EINVAL),
    "a tail without the spans flag": (D(spans=False, tail=T, off=[0, 5]), EINVAL),
    "tail_base + tail_len equal to 0xFFFFFFF0": (D(tail=(0xFFFFFF00, 0xF0), off=[0xFFFFFF00, 0xFFFFFFF0, 3, 4]), ("ok", 3, 4, 1, 0)),
    "tail_base + tail_len equal to 0xFFFFFFF1": (D(tail=(0xFFFFFF00, 0xF1), off=[3, 4]), EINVAL),
    "offsets at and above 2^31": (D(off=[G, G + 10, G - 5, G, 0xFFFFFFF0, 0xFFFFFFFF], pre=[G + 100, G + 200]), ("ok", G - 5, 0xFFFFFFFF, 0, 0)),
    "gather span reaching past tail_base": (D(place="arena", tail=T, off=[0, 5], gather=[1000, 1025, 0, 0, 0, 0]), EINVAL),
    "gather total of 0x7FFFFFF0": (D(place="arena", off=[0, 5], gather=[0, 0x7FFFFFF0, 0, 0, 0, 0]), ("ok", 0, 0x7FFFFFF0, 0, 0x7FFFFFF0)),
    "gather total of 0x7FFFFFF1": (D(place="arena", off=[0, 5], gather=[0, 0x7FFFFFF0, 9, 10, 0, 0]), ETOOBIG),
    "in-arena placement forcing lo = 0": (D(place="arena", tail=T, off=[500, 600, 1024, 1030], nym=[700, 800]), ("ok", 0, 800, 1, 0)),
    "own-buffer placement leaving tail spans unrebased": (D(place="own", tail=T, off=[500, 600, 1024, 1030]), ("ok", 500, 600, 1, 0)),
}
# what the crafted cases must cover, item by item
REQUIRED = ["empty span", "reversed span", "span ending exactly at tail_base", "span starting exactly at tail_base", "span straddling by one byte",
            "tail span ending at the tail's end", "tail span ending one byte past the tail's end", "prefix in the tail, refused",
            "prefix in the tail, permitted", "consecutive offsets with empty first and last messages", "consecutive offsets with a decrease",
            "nothing referencing the arena", "tail_base not a multiple of 64", "a tail without the spans flag",
            "tail_base + tail_len equal to 0xFFFFFFF0", "tail_base + tail_len equal to 0xFFFFFFF1", "offsets at and above 2^31",
            "gather span reaching past tail_base", "gather total of 0x7FFFFFF0", "gather total of 0x7FFFFFF1", "in-arena placement forcing lo = 0",
            "own-buffer placement leaving tail spans unrebased"]


def test_the_crafted_list_is_complete():
    assert sorted(CRAFTED) == sorted(REQUIRED)


def test_crafted_descriptions():
    names = list(CRAFTED)
    got = answers([CRAFTED[k][0] for k in names])
    for k, g in zip(names, got):
        d, want = CRAFTED[k]
        assert g == model(d), k                            # the program against the model, every number
        if isinstance(want, int):                          # ... and both against what the case is there to show
            assert g == ("refused", want), k
        else:
            assert g[:5] == want, k
    # the two placements differ in nothing but lo: where the arena spans land
    assert got[names.index("in-arena placement forcing lo = 0")][5][0] == [500, 600, 1024, 1030]
    assert got[names.index("own-buffer placement leaving tail spans unrebased")][5][0] == [0, 100, 1024, 1030]
    assert got[names.index("empty span")][5][0] == [0, 0, 0, 10]
    assert got[names.index("consecutive offsets with empty first and last messages")][5][:2] == [[10, 10, 20, 30, 30], [0, 0, 5]]


def random_description(rng):
    """Half of them clean - every span where it may lie - and half with mischief in about one span of ten."""
    spans = rng.random() < 0.7
    clean = rng.random() < 0.5
    has_tail = rng.random() < 0.6 and (spans or not clean)
    base = rng.choice([64, 1024, 1 << 20, G, 0xFFFFFF00] + ([] if clean else [1000])) if has_tail else None
    tlen = rng.choice([1, 64, 100, 0xF0] + ([] if clean else [0xF1])) if has_tail else 0
    top = base if has_tail else 0xFFFFFFFF
    prefix_in_tail = rng.random() < 0.2

    def span(may_be_tail=True):
        k = 1.0 if clean or rng.random() < 0.9 else rng.random() * 0.4
        if has_tail and k < 0.2:                           # leaving the tail
            a = base + rng.randrange(0, tlen + 1)
            return a, min(a + rng.randrange(0, tlen + 2), 0xFFFFFFFF)
        if has_tail and k < 0.3:                           # about tail_base
            a = max(base - rng.randrange(0, 3), 0)
            return a, a + rng.randrange(0, 3)
        if k < 0.4:                                        # reversed
            return rng.randrange(1, 2000), 0
        if has_tail and rng.random() < 0.3 and (may_be_tail or not clean):
            a = base + rng.randrange(0, tlen + 1)
            return a, rng.randrange(a, base + tlen + 1)
        a = rng.randrange(0, top + 1)
        return a, rng.randrange(a, min(a + 5000, top) + 1)

    def rows(k, may_be_tail=True):
        if spans:
            return [v for _ in range(k) for v in span(may_be_tail)]
        if k == 0:
            return []
        o = sorted(rng.randrange(0, min(top, 1 << 20) + 1) for _ in range(k + 1))
        if not clean and rng.random() < 0.2:
            o[rng.randrange(len(o))] = rng.randrange(0, 1 << 20)
        return o

    gather = []
    for _ in range(rng.randrange(0, 3)):
        for _ in range(3):
            gather += [0, rng.choice([0x7FFFFFF0, 0x40000000, 0])] if rng.random() < 0.15 and top > 0x7FFFFFF0 else list(span(False))
    return D(place=rng.choice(["arena", "own"]), spans=spans, prefix_in_tail=prefix_in_tail, tail=(base, tlen) if has_tail else None,
             off=rows(rng.randrange(1, 9)), pre=rows(rng.randrange(0, 4), prefix_in_tail),
             nym=[v for _ in range(rng.randrange(0, 3)) for v in span()] if spans else [], gather=gather)


def test_random_descriptions():
    rng = random.Random(20384)
    ds = [random_description(rng) for _ in range(4000)]
    want = [model(d) for d in ds]
    kinds = {w[:2] if w[0] == "refused" else (w[0], w[3]) for w in want}
    assert kinds == {("refused", EINVAL), ("refused", ETOOBIG), ("ok", 0), ("ok", 1)}      # every outcome occurs
    assert sum(w[0] == "ok" for w in want) > 1000
    for d, g, w in zip(ds, answers(ds), want):
        assert g == w, line(d)


def test_the_programs_own_cases():
    """the cases the sanitizer build runs when it is given no script"""
    out = subprocess.run([EXE, "self"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "0 failures", out.stdout + out.stderr
