"""Case lists and helpers of the CKKS evaluator's shape sweep: tests/test_ckks_shapes_cpu.py proves them,
tests/test_ckks_shapes_gpu.py runs them.  Nothing here calls the library under test; the restatements are the existing ones
(tests/_ckks_eval_numpy.py and the modules on it), used as they are.

    A  ladder     every n = 2^1 .. 2^16 on the chain (58, 40): k = 2 and 3 at batch 3 up to 2^13, k = 2 at batch 2 above
    B  depth      n = 256, batch 3, three orders of E.wide_chain(256), every k = 1 .. 8; the as-is order also at every
                  limbs = 1 .. 8 against one key of 8 limbs
    C  alignment  every entry point with buffers one word past a 16-byte boundary, at three shapes; from_i64's staged route
                  over two chunks at (4096, 2, 129)
    D  clamp      (2^16, 6, 2): the smallest shape whose chunk quotient 2^21 / (n k^2) is zero
    E  streams    B runs on a created stream; slot 12 under requests 5, 1, 9; two streams interleaved
"""
import numpy as np

import _ckks_bsgs_numpy as BN
import _ckks_eval_numpy as E

U64, I64 = np.uint64, np.int64
SPEC = (58, 40)
MAX_K = 8

# ---- A ---------------------------------------------------------------------------------------------------------------------------
LADDER = [(1 << L, k, 3) for L in range(1, 14) for k in (2, 3)] + [(1 << L, 2, 2) for L in (14, 15, 16)]
# the keys are the samplers' (and fhe_ckks_rns_relin_key_dev / _galois_key_dev are compared with them) up to here, uniform random
# residues above: the two sampled keys cost 0.15 s of a case at n = 2^13, k = 3 on the GPU box; one key of k = 2 takes the
# restatement 0.2 s at 2^14 and 0.8 s at 2^16 on a host core, two of them as much as the rest of that case (2.0 s at 2^16)
KEY_CUT = 1 << 13


def transform_names(n):
    """the kernel-timer rows (label_tag) of the n-point transforms of a modulus between 2^30 and 2^62: one thread a row below
    16 points, one pass up to 2^13, above that a strided pass of LA stages beside a contiguous one over 2^LB-point blocks,
    LB = max(L - 8, 8)"""
    L = n.bit_length() - 1
    if L < 4:
        return {"ntt_tiny_fwd_%d" % L, "ntt_tiny_inv_%d" % L}
    if L <= 13:
        return {"ntt_fwd_contig_final_%d" % L, "ntt_inv_contig_final_%d" % L}
    LB = max(L - 8, 8)
    return {"ntt_fwd_strided_%d" % (L - LB), "ntt_fwd_contig_final_%d" % LB, "ntt_inv_contig_%d" % LB, "ntt_inv_strided_%d" % (L - LB)}


def reduced(gs, n):
    return [g % (2 * n) for g in gs]


def galois_pair(n):
    """g = 5 and g = 2n - 1 of one hoisted call, reduced modulo 2n (n = 2: the identity and the conjugation)"""
    return [5 % (2 * n), 2 * n - 1]


DIAG = [1, 5]
BABIES, GIANTS = BN.SWEEP


def edge_rows(q, n):
    """the rows of test_edge_residues_and_the_centring that sit at an edge: q - 1 throughout (as evals), and coefficients at
    floor(q / 2) and floor(q / 2) + 1 alternating, in both orders"""
    half = np.array([q // 2, q // 2 + 1] * (n // 2), dtype=U64)
    return np.stack([np.full(n, q - 1, dtype=U64), E.fwd(q, n, half), E.fwd(q, n, half[::-1].copy())])


def planted_ct(mods, n, batch, comps, rng):
    """E.case_ct with the edge rows planted in every component: row 0 is q - 1 throughout, row 1 has its coefficients at the
    centring's edge, row 2 (where the batch has one) the same in the other order"""
    ct = E.case_ct(mods, n, batch, comps, rng)
    for i, q in enumerate(mods):
        rows = edge_rows(q, n)
        for r in range(min(batch, 3)):
            ct[i, :, r] = rows[r]
    return ct


def signed_rows(n, k, batch):
    """from_i64's input with the words -2^63 and 2^63 - 1 planted, as test_entry_points_word_for_word has them"""
    m = np.random.default_rng(n + k).integers(-(1 << 63), (1 << 63) - 1, (batch, n), dtype=np.int64, endpoint=True)
    m[0, :2] = [-(1 << 63), (1 << 63) - 1]
    return m


def random_key(mods, P, n, rng, limbs=None):
    """canonical uniform words in the shape of a switching key [limbs][limbs + 1][2][n], columns 0 .. 7 of every row q - 1: the
    evaluator's word-for-word contract holds for any canonical key words"""
    r = np.random.default_rng(rng)
    allm = list(mods) + [P]
    key = np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) for q in allm]) for _ in range(limbs or len(mods))])
    for i, q in enumerate(allm):
        key[:, i, :, :min(n, 8)] = q - 1
    return key


def weights(mods, shape, rng):
    """canonical Python integers below q_i in the last axis, the first of them q_i - 1"""
    r = np.random.default_rng(rng)
    count = int(np.prod(shape))
    flat = [[int(r.integers(0, q, dtype=np.uint64)) for q in mods] for _ in range(count)]
    flat[0] = [q - 1 for q in mods]
    w = np.empty((count, len(mods)), dtype=object)
    for t, row in enumerate(flat):
        w[t] = row
    return w.reshape(tuple(shape) + (len(mods),)).tolist()


# ---- B ---------------------------------------------------------------------------------------------------------------------------
N_DEPTH, BATCH_DEPTH = 256, 3
ORDERS = ("asis", "reversed", "index3")


def ordered_chain(order):
    """-> (the eight limbs, P, the index of the limb >= 2^62)"""
    mods, P = E.wide_chain(N_DEPTH)
    if order == "reversed":
        mods = mods[::-1]
    elif order == "index3":
        mods = mods[1:4] + mods[:1] + mods[4:]
    else:
        assert order == "asis"
    return mods, P, [i for i, q in enumerate(mods) if q >> 62][0]


DEPTH = [(order, k, k) for order in ORDERS for k in range(1, MAX_K + 1)]                 # (order, limbs, key_limbs)
DEPTH_LOW = [("asis", limbs, MAX_K) for limbs in range(1, MAX_K)]                        # one key of the full chain


def key_sum_folds(k, held, schedule=None):
    """the digits j before which key_sum folds on a limb >= 2^62: j > 0 with (held + j) a multiple of kMacChunk63 = 2"""
    schedule = schedule or (lambda j: (held + j) % 2 == 0)
    return [j for j in range(1, k) if schedule(j)]


def key_sum_peak(q, k, held, schedule=None):
    """the largest value the 128-bit accumulator holds at words q - 1 everywhere: `held` terms on entry, then k terms, folded to
    a canonical word before the digits of key_sum_folds"""
    folds = key_sum_folds(k, held, schedule)
    acc = peak = held * (q - 1) ** 2
    for j in range(k):
        if j in folds:
            acc %= q
        acc += (q - 1) ** 2
        peak = max(peak, acc)
    return peak


# ---- C ---------------------------------------------------------------------------------------------------------------------------
ALIGN_SHAPES = [(16, 2, 3), (1024, 3, 3), (1 << 14, 2, 2)]
ALIGN_MODES = ("all", "inputs", "outputs")
ENTRIES = ("from_i64", "relin_key", "galois_key", "tensor", "relinearize", "mul", "galois_evals", "galois", "diag_sum", "bsgs", "lincomb", "dot")
STAGED = (4096, 2, 129)                       # from_i64 into a misaligned output: chunks of 128 + 1 rows

# ---- D ---------------------------------------------------------------------------------------------------------------------------
CLAMP = (1 << 16, 6, 2)


def chunk_quotient(n, k):
    return E.CHUNK_WORDS // (n * k * k)


def relin_workspace_bytes(n, k, batch):
    """fhe_ckks_rns_workspace_bytes: the key switch's k^2 + 5k + 2 slabs behind the tensor's 3k, or a rescale's 2k"""
    return max((k * k + 8 * k + 2) * E.chunk_rows(n, k, batch), 2 * k * E.chunk_rows(n, k, batch, rescale=True)) * n * 8


# ---- E ---------------------------------------------------------------------------------------------------------------------------
REUSE = (1024, 3, (5, 1, 9))
INTERLEAVE = (1024, 3, 3, 3)                  # n, k, batch, rounds
