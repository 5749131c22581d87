"""Python big-integer statement of typlonk_witness_check (TEST INFRASTRUCTURE ONLY): which gate rows and which copy
constraints a witness fails.  Cells are flat indices x = col * n + row, as the permutation of oracle/plonk_oracle.py."""
import numpy as np

from oracle import bls12_381 as O

R = O.R
SELECTORS = ("q_l", "q_r", "q_o", "q_m", "q_c")


def check(q, perm, cols, pi=()):
    """q: selector name -> n values; perm: 3n successors; cols: three columns of n integers (any representative of the
    residue); pi: the public values (rows len(pi).. are zero).  Returns (failing rows, failing (x, perm[x]) pairs), ascending."""
    n = len(cols[0])
    a, b, c = cols
    gate = [j for j in range(n)
            if (q["q_l"][j] * a[j] + q["q_r"][j] * b[j] - q["q_o"][j] * c[j] + q["q_m"][j] * a[j] * b[j] + q["q_c"][j]
                + (pi[j] if j < len(pi) else 0)) % R]
    cell = lambda x: cols[x // n][x % n]   # noqa: E731
    copy = [(x, perm[x]) for x in range(3 * n) if (cell(x) - cell(perm[x])) % R]
    return gate, copy


def satisfied(q, perm, cols, pi=()):
    gate, copy = check(q, perm, cols, pi)
    return not gate and not copy


def chain_with_pi(log_n, pi=(), x0=3, blinders=None):
    """the squaring chain of oracle/plonk_oracle.py under public values: x_{j+1} = x_j^2 + pi_j (the gate row reads
    q_m a b - q_o c + PI = 0).  Returns (n, cols, q, perm)."""
    from oracle import plonk_oracle as PO

    n, cols, q, perm = PO.squaring_chain(log_n, x0, blinders)
    g, x, xs = n - 3, x0 % R, []
    for j in range(g + 1):
        xs.append(x)
        x = (x * x + (pi[j] if j < len(pi) else 0)) % R
    cols = [xs[:g] + cols[0][g:], xs[:g] + cols[1][g:], xs[1:g + 1] + cols[2][g:]]
    return n, cols, q, perm


# ---- the raw-word view -----------------------------------------------------------------------------------------------------------
# The device reads Montgomery words: a datum whose four words spell the integer w < 2^256 stands for the residue w * 2^-256
# mod r, whether or not w is below r.  The functions below take and return numpy object arrays (Python integers inside).
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
_WORD = (1 << 64) - 1


def _obj(values):
    out = np.empty(len(values), dtype=object)
    out[:] = values if isinstance(values, list) else list(values)
    return out


def raw_of(residues):
    """residues -> their canonical raw values v * 2^256 mod r"""
    return _obj(residues) % R * MONT % R


def residues_of(raw):
    """raw values below 2^256 (any representative) -> the residues they stand for"""
    return _obj(raw) * MONT_INV % R


def raw_words(raw):
    """raw values below 2^256 -> the (len, 4) uint64 array the C ABI takes, as they are (no reduction)"""
    raw = _obj(raw)
    out = np.empty((len(raw), 4), dtype=np.uint64)
    for i in range(4):
        out[:, i] = ((raw >> (64 * i)) & _WORD).astype(np.uint64)
    return out


def words_raw(words):
    """the inverse of raw_words"""
    w = np.asarray(words, dtype=np.uint64).astype(object)
    return w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192)


def mont_words(residues):
    """helpers.fr_pack, vectorised"""
    return raw_words(raw_of(residues))


def check_raw(q, perm, raw_cols, raw_pi=()):
    """check() on a witness given as raw values"""
    return check(q, perm, [residues_of(c).tolist() for c in raw_cols], residues_of(raw_pi).tolist())


# ---- random circuits -------------------------------------------------------------------------------------------------------------
def random_circuit(log_n, seed, pi_len=0):
    """A circuit with full-range selectors over an arbitrary permutation, and an honest witness of it.  A seeded shuffle of
    the 3n cells is cut into cycles: a fixed point, a 2-cycle and one of min(3n / 4, 200..400) cells first, then lengths drawn
    from {1, 2, 3..8, 9..40, 200..400} until the cells run out.  Every cycle holds one random residue; q_l, q_r, q_o, q_m
    and the public values are uniform in [0, r), and q_c = -(q_l a + q_r b - q_o c + q_m a b + PI) row by row.
    Returns (n, cols, q, perm, pi) in the form check() takes."""
    import random

    n = 1 << log_n
    if pi_len > n:
        raise ValueError("more public values than rows")
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    order = nrng.permutation(3 * n)
    lengths, left = [], 3 * n
    for want in (1, 2, min(3 * n // 4, rng.randrange(200, 401))):
        lengths.append(want)
        left -= want
    while left:
        kind = rng.randrange(5)
        want = (1, 2, rng.randrange(3, 9), rng.randrange(9, 41), rng.randrange(200, 401))[kind]
        lengths.append(min(want, left))
        left -= lengths[-1]
    lengths = np.array(lengths, dtype=np.int64)
    starts = np.cumsum(lengths) - lengths
    # the successor of the cell at position p of the shuffle: the one at p + 1, the cycle's first from its last
    nxt = np.arange(1, 3 * n + 1, dtype=np.int64)
    nxt[starts + lengths - 1] = starts
    perm = np.empty(3 * n, dtype=np.int64)
    perm[order] = order[nxt]
    value = np.empty(3 * n, dtype=object)
    value[order] = _obj([rng.randrange(R) for _ in lengths])[np.repeat(np.arange(len(lengths)), lengths)]
    a, b, c = value[:n], value[n:2 * n], value[2 * n:]
    q = {name: _obj([rng.randrange(R) for _ in range(n)]) for name in SELECTORS[:4]}
    pi = [rng.randrange(R) for _ in range(pi_len)]
    pub = _obj(pi + [0] * (n - pi_len))
    q["q_c"] = -(q["q_l"] * a + q["q_r"] * b - q["q_o"] * c + q["q_m"] * a * b + pub) % R
    return n, [a.tolist(), b.tolist(), c.tolist()], {name: v.tolist() for name, v in q.items()}, perm.tolist(), pi


def cycles_of(perm):
    """the cycles of a permutation, each from its lowest cell on"""
    seen, out = [False] * len(perm), []
    for x in range(len(perm)):
        if not seen[x]:
            cyc = []
            while not seen[x]:
                seen[x] = True
                cyc.append(x)
                x = perm[x]
            out.append(cyc)
    return out
