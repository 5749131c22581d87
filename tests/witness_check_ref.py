"""Python big-integer statement of typlonk_witness_check (TEST INFRASTRUCTURE ONLY): which gate rows and which copy
constraints a witness fails.  Cells are flat indices x = col * n + row, as the permutation of oracle/plonk_oracle.py."""
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
