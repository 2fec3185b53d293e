"""The launch classes of the gadget kernels of digit32.hip (digit_mac32_kernel<LP, 4, SRC32_G*>, digit_tail32_kernel),
enumerated without a device: a Python restatement of the host's split, the class of a call, the universe of classes an
admitted shape can reach on the batch ladder, and CASES, the list that tests/test_gadget_shapes_gpu.py runs.  The
restatement only plans the sweep: every comparison of the sweep is against an independent reference, whatever the split
really is, and the batch ladder has both sides of every power-of-two threshold the split can have."""
import functools

import pytest

from test_gadget_cpu import PA, PB, admitted

SIZES = (256, 512, 1024, 2048, 4096)
MODES = ("gadget", "gcmux", "gsel")        # SRC32_GADGET + EPI32_TORUS, SRC32_GCMUX + EPI32_CMUX, SRC32_GSEL + EPI32_SEL
# 1 .. 9, both sides of every batch = slots / (2 p) (slots 2048 / 512 / 256, p = 1 .. 64: 1024 down to 2), and 2049
LADDER = tuple(sorted(set(range(1, 10)) | {t + d for t in (16, 32, 64, 128, 256, 512, 1024) for d in (-1, 0, 1)} | {2049}))


def ext32_units(log_n):
    """digit32.hip:636 ext32_units = Mac32Cfg<LP>::W (digit32.hip:173-179: TH / TPB): digits per step"""
    return (2 if log_n == 12 else 4096 >> log_n) if 8 <= log_n <= 12 else 0


def ext32_gadget_split(n, batch, T):
    """digit32.hip:649-658 -> (parts, tpp)"""
    W = ext32_units(n.bit_length() - 1)
    steps = (T + W - 1) // W
    slots = 2048 if n <= 1024 else 512 if n == 2048 else 256
    p = 1
    while p < steps and batch * p * 2 <= slots:
        p *= 2
    per = (steps + p - 1) // p
    return (steps + per - 1) // per, per * W


def tail_units(n):
    """ContigCfg<LP>::W (ntt_rounds.hpp:525-526): output rows per workgroup of digit_tail32_kernel, 256 / (n / 16)"""
    return 4096 // n


def max_b(n, l):
    """the largest admitted log_beta of (n, l), 0 if none (test_gadget_cpu.admitted restates ext32_gadget_supported)"""
    return max((b for b in range(1, 65) if admitted(n, 1, b, l)), default=0)


def _bucket(x, edges):
    for i, e in enumerate(edges):
        if x <= e:
            return i
    return len(edges)


def launch_shape(n, l, batch):
    W = ext32_units(n.bit_length() - 1)
    T = 2 * l                                                     # k = 1
    parts, tpp = ext32_gadget_split(n, batch, T)
    return dict(W=W, T=T, steps=(T + W - 1) // W, parts=parts, per=tpp // W, tpp=tpp, last=T - (parts - 1) * tpp)


def launch_class(n, l, batch):
    """(n, steps {1, 2, 3, >= 4}, parts {1, 2, 3, 4, 5-8, >= 9}, per {1, 2, >= 3}, partial last step, short last part,
    T < W, 2 batch a multiple of the tail's units); the mode is the last coordinate of a class, added by classes_of"""
    s = launch_shape(n, l, batch)
    return (n, _bucket(s["steps"], (1, 2, 3)), _bucket(s["parts"], (1, 2, 3, 4, 8)), _bucket(s["per"], (1, 2)), s["T"] % s["W"] != 0,
            s["last"] != s["tpp"], s["T"] < s["W"], (2 * batch) % tail_units(n) == 0)


def classes_of(n, l, batch):
    return {launch_class(n, l, batch) + (m,) for m in MODES}      # every case runs the three entry points


@functools.lru_cache(None)
def universe():
    """class -> the (l, batch) that reach it, over every admitted (n, b, l) (the class does not depend on b, and b = 1
    admits every l that any b does)"""
    out = {}
    for n in SIZES:
        for l in range(1, 65):
            if admitted(n, 1, 1, l):
                for batch in LADDER:
                    for c in classes_of(n, l, batch):
                        out.setdefault(c, []).append((l, batch))
    return out


@functools.lru_cache(None)
def _cover():
    """a greedy cover of the universe: per n, the l that reaches the most uncovered classes per unit of l (the reference
    costs ~ l products per row), then the ladder batches of that l that each add a class.  -> [(n, l, [batch ...])]"""
    out = []
    for n in SIZES:
        need = {c[:-1] for c in universe() if c[0] == n}
        ls = [l for l in range(1, 65) if admitted(n, 1, 1, l)]
        while need:
            _, l = max((len({launch_class(n, l, b) for b in LADDER} & need) / l, -l) for l in ls)
            l = -l
            batches, got = [], set()
            for b in LADDER:
                c = launch_class(n, l, b)
                if c in need and c not in got:
                    got.add(c)
                    batches.append(b)
            assert got
            need -= got
            out.append((n, l, batches))
    return out


def _cases():
    """(n, b, l, batch): every batch of the cover at the largest admitted b, then one more case per (n, l) with b = 1"""
    out = []
    for n, l, batches in _cover():
        out += [(n, max_b(n, l), l, batch) for batch in batches]
        if max_b(n, l) != 1:
            out.append((n, 1, l, batches[0]))
    return out


CASES = _cases()
# every key word 2^64 - 1 and every digit -2^(b-1) at the admission edge, per n (l = 2 and 3 at their largest b): the
# construction of test_gadget_gpu.test_gadget_external_product_worst_case_at_the_edge
WORST = [(n, max_b(n, l), l) for n in SIZES for l in (2, 3)]


def test_the_case_list_leaves_out_no_class_of_the_universe():
    covered = set()
    for n, b, l, batch in CASES:
        covered |= classes_of(n, l, batch)
    missing = sorted(set(universe()) - covered)
    assert len(missing) == 0, missing[:10]
    assert covered == set(universe())                              # and no case lies outside the ladder or the rule
    # the universe is what the issue counted: several hundred classes, every n, mode and bucket present
    assert len(universe()) >= 300
    for pos, values in ((0, set(SIZES)), (1, {0, 1, 2, 3}), (2, {0, 1, 2, 3, 4, 5}), (3, {0, 1, 2}), (4, {False, True}),
                        (5, {False, True}), (6, {False, True}), (7, {False, True}), (8, set(MODES))):
        assert {c[pos] for c in universe()} == values, pos
    for n in SIZES:
        # parts from 1 to beyond 8, except n = 256: T <= 128 is at most 8 steps of 16 digits
        assert {c[2] for c in universe() if c[0] == n} == ({0, 1, 2, 3, 4} if n == 256 else {0, 1, 2, 3, 4, 5}), n
    assert max(launch_shape(4096, 64, 1)["parts"], launch_shape(256, 64, 1)["parts"]) == 64


def test_every_case_is_admitted_at_full_digit_width_with_one_more_at_b_1():
    seen = {}
    for n, b, l, batch in CASES:
        assert batch in LADDER and n in SIZES
        assert admitted(n, 1, b, l)
        assert 2 * l * n * ((1 << 32) - 1) * (1 << (b - 1)) < PA * PB // 2 + 1      # the worst half-sum is below pA pB / 2
        assert 2 * 2 * l * n * ((1 << 32) - 1) * (1 << (b - 1)) < PA * PB
        seen.setdefault((n, l), set()).add(b)
    for (n, l), bs in seen.items():
        top = max_b(n, l)
        assert bs == {top, 1}, (n, l, bs)
        assert top == 64 // l or not admitted(n, 1, top + 1, l)
    for n, b, l in WORST:
        assert admitted(n, 1, b, l) and not admitted(n, 1, b + 1, l)
    # the values test_gadget_cpu.test_admission_edges pins
    assert (max_b(1024, 2), max_b(1024, 3), max_b(4096, 2)) == (10, 10, 8)
    assert [max_b(n, 1) for n in SIZES] == [13, 12, 11, 10, 9] and all(max_b(n, 64) == 1 for n in SIZES)


@pytest.mark.parametrize("n,batch,T,want", [
    (1024, 1024, 6, (2, 4)), (1024, 1025, 6, (1, 8)),             # the threshold the bootstrap tests cross
    (2048, 256, 4, (2, 2)), (2048, 257, 4, (1, 4)),
    (4096, 1, 128, (64, 2)), (4096, 2, 128, (64, 2)), (4096, 3, 128, (64, 2)), (4096, 5, 128, (32, 4)), (4096, 129, 128, (1, 128)),
    (256, 1, 2, (1, 16)), (256, 1, 128, (8, 16)), (512, 5, 10, (2, 8)), (1024, 7, 14, (4, 4)), (1024, 600, 22, (2, 12)),
    (1024, 300, 22, (3, 8)),                                      # steps 6, p 4 -> per 2 -> three parts
])
def test_the_restated_split_at_known_points(n, batch, T, want):
    assert ext32_gadget_split(n, batch, T) == want
    parts, tpp = want
    assert (parts - 1) * tpp < T <= parts * tpp                    # no part is empty
