"""Python big-integer statement of typlonk_witness_solve (TEST INFRASTRUCTURE ONLY): the three wire columns of a witness from a
handful of assigned cells and the public values -- the contract of include/typlonk.h, stated without the library's data
structures -- and the circuits the tests solve.  Cells are flat indices x = col * n + row.

  row j is DRIVEN iff q_o[j] != 0 mod r; a class (a cycle of perm) is driven iff it holds the c cell 2n + j of a driven row, its
  driver is the lowest such row; every other class is free and takes its assigned value, or 0.  A driven row's c cell gets
  (q_l a + q_r b + q_m a b + q_c + PI) / q_o, a and b being the values of the classes of its a and b cells; every other cell gets
  its class's value (the driver's c)."""
import random

import witness_check_ref as W

R = W.R
FREE = 1 << 31
NARROW, RUN_CUT = 256, 65536


class Unsolvable(ValueError):
    """the rows' dependencies have a cycle; .row = the lowest row that cannot be scheduled"""

    def __init__(self, row):
        super().__init__(f"row {row} cannot be scheduled")
        self.row = row


def driven_rows(q):
    return [v % R != 0 for v in q["q_o"]]


def sources(q, perm):
    """(src, number of free classes): src[x] = the driven row whose c cell holds x's value, or FREE | slot; slots are numbered
    by the lowest cell of their class"""
    n = len(q["q_o"])
    driven, src, free = driven_rows(q), [None] * (3 * n), 0
    for cyc in W.cycles_of(perm):
        drivers = [x - 2 * n for x in cyc if x >= 2 * n and driven[x - 2 * n]]
        s = min(drivers) if drivers else FREE | free
        free += not drivers
        for x in cyc:
            src[x] = s
    for j in range(n):
        if driven[j]:
            src[2 * n + j] = j
    return src, free


def levels(q, perm):
    """level[j] = 1 + the larger level of the sources of row j's a and b cells (a free source: 0) for a driven row, 0 for an
    undriven one.  By depth-first search; Unsolvable names the lowest row that lies on, or depends on, a cycle."""
    n = len(q["q_o"])
    src, _ = sources(q, perm)
    driven = driven_rows(q)
    deps = lambda j: [s for s in (src[j], src[n + j]) if not s & FREE]   # noqa: E731
    level, state, bad = [0] * n, [0] * n, set()      # state: 0 new, 1 open, 2 done
    for root in range(n):
        if not driven[root] or state[root]:
            continue
        stack = [(root, iter(deps(root)))]
        state[root] = 1
        while stack:
            j, it = stack[-1]
            for d in it:
                if state[d] == 0:
                    state[d] = 1
                    stack.append((d, iter(deps(d))))
                    break
                if state[d] == 1 or d in bad:
                    bad.add(j)
            else:
                stack.pop()
                state[j] = 2
                if any(d in bad for d in deps(j)):
                    bad.add(j)
                level[j] = 1 + max([level[d] for d in deps(j)], default=0)
    if bad:
        raise Unsolvable(min(bad))
    return level


def plan(q, perm, narrow=NARROW, run_cut=RUN_CUT):
    """what tests/cpp/solve_plan_host prints for the same circuit"""
    src, free = sources(q, perm)
    try:
        level = levels(q, perm)
    except Unsolvable as e:
        return {"status": 2, "bad": e.row}
    depth = max(level, default=0)
    order = sorted((j for j in range(len(level)) if level[j]), key=lambda j: (level[j], j))
    level_off = [0] * (depth + 1)
    for j in order:
        level_off[level[j]] += 1
    for l in range(depth):
        level_off[l + 1] += level_off[l]
    schedule = []
    for l in range(depth):
        width = level_off[l + 1] - level_off[l]
        if width > narrow:
            schedule.append([l, 1, 1])
        elif schedule and not schedule[-1][2] and schedule[-1][1] < run_cut:
            schedule[-1][1] += 1
        else:
            schedule.append([l, 1, 0])
    return {"status": 0, "bad": 0, "driven_rows": len(order), "free_classes": free, "depth": depth, "launches": len(schedule) + 1,
            "src": src, "level": level, "order": order, "level_off": level_off, "schedule": schedule}


def solve(q, perm, assigned, pi=()):
    """assigned: {cell: value} over free classes, at most one cell per class -> the three columns"""
    n = len(q["q_o"])
    src, free = sources(q, perm)
    slot = [0] * free
    for x, v in assigned.items():
        if not src[x] & FREE:
            raise ValueError(f"cell {x} lies in a driven class")
        slot[src[x] & ~FREE] = v % R
    level = levels(q, perm)
    c = [0] * n
    value = lambda s: slot[s & ~FREE] if s & FREE else c[s]   # noqa: E731
    for j in sorted((j for j in range(n) if level[j]), key=lambda j: level[j]):
        a, b = value(src[j]), value(src[n + j])
        num = q["q_l"][j] * a + q["q_r"][j] * b + q["q_m"][j] * a * b + q["q_c"][j] + (pi[j] if j < len(pi) else 0)
        c[j] = num * pow(q["q_o"][j], -1, R) % R
    cells = [value(s) for s in src]
    return [cells[:n], cells[n:2 * n], cells[2 * n:]]


def solve_many(q, perm, wits):
    """[solve(q, perm, assigned, pi) for assigned, pi in wits], with the work that belongs to the circuit (the sources, the
    levels, the order of the rows, one modular inverse per driven row) done once for all of them"""
    n = len(q["q_o"])
    src, free = sources(q, perm)
    level = levels(q, perm)
    order = sorted((j for j in range(n) if level[j]), key=lambda j: level[j])
    rows = [(j, src[j], src[n + j], q["q_l"][j], q["q_r"][j], q["q_m"][j], q["q_c"][j], pow(q["q_o"][j], -1, R)) for j in order]
    out = []
    for assigned, pi in wits:
        slot = [0] * free
        for x, v in assigned.items():
            if not src[x] & FREE:
                raise ValueError(f"cell {x} lies in a driven class")
            slot[src[x] & ~FREE] = v % R
        c = [0] * n
        value = lambda s: slot[s & ~FREE] if s & FREE else c[s]   # noqa: E731
        for j, sa, sb, ql, qr, qm, qc, inv in rows:
            a, b = value(sa), value(sb)
            c[j] = (ql * a + qr * b + qm * a * b + qc + (pi[j] if j < len(pi) else 0)) * inv % R
        cells = [value(s) for s in src]
        out.append([cells[:n], cells[n:2 * n], cells[2 * n:]])
    return out


# ---- circuits ------------------------------------------------------------------------------------------------------------------
BLINDERS = [[(7 * i + 3 * j + 11) % R for j in range(3)] for i in range(3)]


def blinding_cells(n, blinders=BLINDERS):
    """{cell: value} of the three blinding rows n - 3 .. n - 1"""
    return {i * n + n - 3 + k: blinders[i][k] for i in range(3) for k in range(3)}


def chain(log_n, pi=(), x0=3):
    """(b) the squaring chain under public values (witness_check_ref.chain_with_pi): (n, q, perm, assigned, honest columns).
    One input (cell a_0), n - 3 levels of one row each."""
    n, cols, q, perm = W.chain_with_pi(log_n, pi, x0, BLINDERS)
    assigned = {0: x0 % R}
    assigned.update(blinding_cells(n))
    return n, q, perm, assigned, cols


def readme():
    """(c) the README circuit a*a + b*b == c*c (oracle/frontend.py): (n, q, perm, input cells).  The inputs are the a cells of
    the three squarings."""
    from oracle import frontend as F

    def run(v):
        a, b, c = v[0] * v[0], v[1] * v[1], v[2] * v[2]
        (a + b).assert_eq(c)

    rows, _, sel, perm = F.compile_circuit(run, 3)
    q = {name: [row[k] for row in sel] for k, name in enumerate(W.SELECTORS)}
    return rows, q, perm, [0, 1, 2], run


def layered(log_n, seed, widths, pi=(), ties=(2, 2), inputs=6):
    """(a) a circuit built level by level and then shuffled.  Level k holds widths[k] driven rows; a row's b operand is an output
    of level k - 1 (an input at level 0) and its a operand any earlier output or input, so the row's level is exactly k + 1.
    q_l, q_r, q_o, q_m, q_c are uniform non-zero on driven rows.  The first 2 * (ties[0] + ties[1]) rows of the last level are
    pairs whose c cells share a class: ties[0] pairs compute equal values (same operands and selectors, q_c adjusted for the
    public values), ties[1] pairs unequal ones; no driven row reads them.  The rows that are left of the first n - 3 are undriven
    (q_o = 0): their operands are any variables, every second one's c cell joins a variable's class, and their q_c closes them on
    the honest witness.  The last input is never assigned (it reads 0); the last three rows are free blinding rows (pi must be 0
    there).  Row order is shuffled.
    Returns a dict: n, q, perm, assigned, pi, cols (the honest columns, by solve()), level (the level every row was built for),
    unequal (the sorted cells of the classes that hold two different computed values), undriven (rows)."""
    rng = random.Random(seed)
    n = 1 << log_n
    g = n - 3
    n_driven, n_tie = sum(widths), 2 * sum(ties)
    assert n_driven <= g and widths[-1] >= n_tie and all(p % R == 0 for p in pi[g:])
    pos = list(range(g))
    rng.shuffle(pos)                                   # logical row -> table row
    q = {name: [0] * n for name in W.SELECTORS}
    classes = [[] for _ in range(inputs)]              # variable -> its cells
    pool, prev, built_level = list(range(inputs)), list(range(inputs)), [0] * n
    pub = lambda j: pi[j] if j < len(pi) else 0   # noqa: E731
    row, sinks, unequal_classes = 0, [], []
    for k, width in enumerate(widths):
        outs, last = [], k == len(widths) - 1
        for i in range(width):
            j = pos[row]
            row += 1
            built_level[j] = k + 1
            twin = last and i < n_tie and i % 2 == 1   # the second row of a tied pair
            if twin:
                va, vb = ops
            else:
                va, vb = rng.choice(pool), rng.choice(prev)
                ops = (va, vb)
            classes[va].append(j)
            classes[vb].append(n + j)
            if twin and i < 2 * ties[0]:               # equal: the same numerator and q_o as the first row
                for name in W.SELECTORS:
                    q[name][j] = q[name][first]
                q["q_c"][j] = (q["q_c"][first] + pub(first) - pub(j)) % R
            else:
                for name in W.SELECTORS:
                    q[name][j] = rng.randrange(1, R)
            if twin:
                classes[out].append(2 * n + j)
                if i >= 2 * ties[0]:
                    unequal_classes.append(out)
            else:
                out, first = len(classes), j
                classes.append([2 * n + j])
                if last and i < n_tie:
                    sinks.append(out)
                else:
                    outs.append(out)
        pool += outs
        prev = outs or prev
    undriven = []
    for i in range(g - n_driven):
        j = pos[row]
        row += 1
        undriven.append(j)
        for col in range(2):
            classes[rng.choice(pool + sinks)].append(col * n + j)
        if i % 2:
            classes[rng.choice(pool + sinks)].append(2 * n + j)
        for name in ("q_l", "q_r", "q_m"):
            q[name][j] = rng.randrange(1, R)
    perm = list(range(3 * n))
    for cells in classes:
        for u, v in zip(cells, cells[1:] + cells[:1]):
            perm[u] = v
    assigned = {classes[v][0]: rng.randrange(1, R) for v in range(inputs - 1) if classes[v]}
    assigned.update(blinding_cells(n))
    cols = solve(q, perm, assigned, pi)
    for j in undriven:
        a, b = cols[0][j], cols[1][j]
        q["q_c"][j] = -(q["q_l"][j] * a + q["q_r"][j] * b + q["q_m"][j] * a * b + pub(j)) % R
    unequal = sorted(x for v in unequal_classes for x in classes[v])
    return {"n": n, "q": q, "perm": perm, "assigned": assigned, "pi": list(pi), "cols": cols, "level": built_level,
            "unequal": unequal, "undriven": sorted(undriven)}


def public_values(n, pi_len, seed, zero_rows=()):
    """pi_len public values, zero on the blinding rows and on zero_rows"""
    rng = random.Random(seed)
    skip = set(zero_rows) | {n - 3, n - 2, n - 1}
    return [0 if j in skip else rng.randrange(1, R) for j in range(pi_len)]
