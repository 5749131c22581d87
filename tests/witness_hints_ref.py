"""Python big-integer statement of typlonk_circuit_set_hints and of a solve under hints (TEST INFRASTRUCTURE ONLY): what
tests/witness_solve_ref.py states, with the free classes a hint computes.  A hint is a tuple (kind, dst, src, shift, width):

  the free class of cell dst takes f(the value the solve writes to cell src): INV0 = 1 / v, and 0 for v = 0; BITS = bits
  [shift, shift + width) of the integer v in [0, r).  src[x] = HINT | h for every cell x of the class of hint h's dst.  A hint's
  level is 1 + the level of its source (a free, unhinted source: 0); a row counts a hinted source with the hint's level.  The
  level lists hold the rows, ascending, then the hints (HINT | h), ascending."""
import random

import witness_check_ref as W
import witness_solve_ref as S

R, FREE, NARROW, RUN_CUT = S.R, S.FREE, S.NARROW, S.RUN_CUT
HINT = 3 << 30
INV0, BITS = 1, 2
# the statuses of csrc/solve_plan.hpp
OK, BAD_PERM, CYCLE, HINT_KIND, HINT_CELL, HINT_RANGE, HINT_DRIVEN, HINT_CLASH, HINT_CYCLE = range(9)


def is_hint(s):
    return s & HINT == HINT


class Refused(ValueError):
    """a refused set of hints: .status as solve_plan.hpp numbers it, .bad = the hint (the row for CYCLE), .other = the lower hint of a
    clash"""

    def __init__(self, status, bad, other=0):
        super().__init__(f"status {status} at {bad}")
        self.status, self.bad, self.other = status, bad, other


def sources(q, perm, hints):
    """(src, number of free classes), hinted classes included in the count: they keep their slot number, unused"""
    n = len(q["q_o"])
    src, free = S.sources(q, perm)
    member = {}
    for cyc in W.cycles_of(perm):
        for x in cyc:
            member[x] = cyc
    for h, (kind, dst, frm, shift, width) in enumerate(hints):
        if kind not in (INV0, BITS):
            raise Refused(HINT_KIND, h)
        if dst >= 3 * n or frm >= 3 * n:
            raise Refused(HINT_CELL, h)
        if kind == BITS and not (1 <= width <= 64 and 0 <= shift <= 254):
            raise Refused(HINT_RANGE, h)
        if any(not src[x] & FREE for x in member[dst]):
            raise Refused(HINT_DRIVEN, h)
        if is_hint(src[dst]):
            raise Refused(HINT_CLASH, h, src[dst] & ~HINT)
        for x in member[dst]:
            src[x] = HINT | h
    return src, free


def levels(q, perm, hints):
    """(level of every row, level of every hint), by relaxation: a node gets its level once all it reads have theirs.  What is
    left lies on, or depends on, a cycle: Refused(CYCLE, lowest such row), or Refused(HINT_CYCLE, lowest such hint) if there is no
    such row."""
    n = len(q["q_o"])
    src, _ = sources(q, perm, hints)
    driven = S.driven_rows(q)
    node = lambda s: None if s & FREE and not is_hint(s) else (n + (s & ~HINT) if is_hint(s) else s)   # noqa: E731
    deps = {j: [node(src[j]), node(src[n + j])] for j in range(n) if driven[j]}
    deps.update({n + h: [node(src[t[2]])] for h, t in enumerate(hints)})
    deps = {v: [d for d in ds if d is not None] for v, ds in deps.items()}
    lv, todo = {}, set(deps)
    while todo:
        ready = [v for v in todo if all(d in lv for d in deps[v])]
        if not ready:
            rows = [v for v in todo if v < n]
            raise Refused(CYCLE, min(rows)) if rows else Refused(HINT_CYCLE, min(todo) - n)
        new = {v: 1 + max([lv[d] for d in deps[v]], default=0) for v in ready}
        lv.update(new)
        todo -= set(ready)
    return [lv.get(j, 0) for j in range(n)], [lv[n + h] for h in range(len(hints))]


def plan(q, perm, hints, narrow=NARROW, run_cut=RUN_CUT):
    """what tests/cpp/solve_hints_host prints for the same circuit and hints"""
    try:
        src, free = sources(q, perm, hints)
        level, hint_level = levels(q, perm, hints)
    except Refused as e:
        return {"status": e.status, "bad": e.bad, "other": e.other}
    n = len(level)
    depth = max(level + hint_level, default=0)
    entries = [(level[j], 0, j, j) for j in range(n) if level[j]] + [(hint_level[h], 1, h, HINT | h) for h in range(len(hints))]
    entries.sort()
    order = [e[3] for e in entries]
    level_off = [0] * (depth + 1)
    for e in entries:
        level_off[e[0]] += 1
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
    return {"status": 0, "bad": 0, "other": 0, "driven_rows": sum(1 for v in level if v), "free_classes": free, "depth": depth,
            "launches": len(schedule) + 1, "src": src, "level": level, "hint_level": hint_level, "order": order,
            "level_off": level_off, "schedule": schedule}


def info(q, perm, hints):
    """what typlonk_witness_solve_plan reports"""
    p = plan(q, perm, hints)
    return {k: p[k] for k in ("driven_rows", "free_classes", "depth", "launches")}


def hint_value(kind, v, shift, width):
    v %= R
    if kind == INV0:
        return pow(v, -1, R) if v else 0
    return (v >> shift) & ((1 << width) - 1)


def solve(q, perm, hints, assigned, pi=()):
    """assigned: {cell: value} over free, unhinted classes -> the three columns"""
    n = len(q["q_o"])
    src, free = sources(q, perm, hints)
    slot = [0] * free
    for x, v in assigned.items():
        if not src[x] & FREE or is_hint(src[x]):
            raise ValueError(f"cell {x} lies in a computed class")
        slot[src[x] & ~FREE] = v % R
    level, hint_level = levels(q, perm, hints)
    c, hv = [0] * n, [0] * len(hints)
    value = lambda s: (hv[s & ~HINT] if is_hint(s) else slot[s & ~FREE]) if s & FREE else c[s]   # noqa: E731
    nodes = [(level[j], j) for j in range(n) if level[j]] + [(hint_level[h], n + h) for h in range(len(hints))]
    for _, v in sorted(nodes):
        if v >= n:
            kind, _, frm, shift, width = hints[v - n]
            hv[v - n] = hint_value(kind, value(src[frm]), shift, width)
            continue
        j = v
        a, b = value(src[j]), value(src[n + j])
        num = q["q_l"][j] * a + q["q_r"][j] * b + q["q_m"][j] * a * b + q["q_c"][j] + (pi[j] if j < len(pi) else 0)
        c[j] = num * pow(q["q_o"][j], -1, R) % R
    cells = [value(s) for s in src]
    return [cells[:n], cells[n:2 * n], cells[2 * n:]]


def solve_many(q, perm, hints, wits):
    """[solve(q, perm, hints, assigned, pi) for assigned, pi in wits], with the work that belongs to the circuit and its hints
    (the sources, the levels, the order of rows and hints, one modular inverse per driven row) done once for all of them"""
    n = len(q["q_o"])
    src, free = sources(q, perm, hints)
    level, hint_level = levels(q, perm, hints)
    nodes = sorted([(level[j], j) for j in range(n) if level[j]] + [(hint_level[h], n + h) for h in range(len(hints))])
    steps = []
    for _, v in nodes:
        if v >= n:
            kind, _, frm, shift, width = hints[v - n]
            steps.append((v, src[frm], kind, shift, width))
        else:
            steps.append((v, src[v], src[n + v], q["q_l"][v], q["q_r"][v], q["q_m"][v], q["q_c"][v], pow(q["q_o"][v], -1, R)))
    out = []
    for assigned, pi in wits:
        slot = [0] * free
        for x, v in assigned.items():
            if not src[x] & FREE or is_hint(src[x]):
                raise ValueError(f"cell {x} lies in a computed class")
            slot[src[x] & ~FREE] = v % R
        c, hv = [0] * n, [0] * len(hints)
        value = lambda s: (hv[s & ~HINT] if is_hint(s) else slot[s & ~FREE]) if s & FREE else c[s]   # noqa: E731
        for step in steps:
            if step[0] >= n:
                v, frm, kind, shift, width = step
                hv[v - n] = hint_value(kind, value(frm), shift, width)
            else:
                j, sa, sb, ql, qr, qm, qc, inv = step
                a, b = value(sa), value(sb)
                c[j] = (ql * a + qr * b + qm * a * b + qc + (pi[j] if j < len(pi) else 0)) * inv % R
        cells = [value(s) for s in src]
        out.append([cells[:n], cells[n:2 * n], cells[2 * n:]])
    return out


# ---- circuits ------------------------------------------------------------------------------------------------------------------
def _perm_of(n, classes):
    perm = list(range(3 * n))
    for cells in classes:
        for u, v in zip(cells, cells[1:] + cells[:1]):
            perm[u] = v
    return perm


def _zero_q(n):
    return {name: [0] * n for name in W.SELECTORS}


def range_check(log_n, k):
    """x + y < 2^k.  Row 0: s = x + y.  Rows 1 .. k: the boolean rows b (b - 1) = 0 of the bits of s, bit i hinted from the c cell
    of row 0.  Rows k + 1 .. 2k - 1: acc + 2^i b_i; the last one's c cell is tied to s.  (n, q, perm, hints, input cells x, y)"""
    n = 1 << log_n
    assert 2 * k <= n - 3 and k >= 2
    q = _zero_q(n)
    q["q_l"][0] = q["q_r"][0] = q["q_o"][0] = 1
    bit = [[1 + i, n + 1 + i] for i in range(k)]
    for i in range(k):
        q["q_m"][1 + i], q["q_l"][1 + i] = 1, R - 1
    classes = [[2 * n, 2 * n + 2 * k - 1]]
    for t in range(k - 1):
        j = k + 1 + t
        q["q_l"][j], q["q_r"][j], q["q_o"][j] = 1, 1 << (t + 1), 1
        if t == 0:
            bit[0].append(j)
        else:
            classes.append([2 * n + j - 1, j])
        bit[t + 1].append(n + j)
    hints = [(BITS, 1 + i, 2 * n, i, 1) for i in range(k)]
    return n, q, _perm_of(n, classes + bit), hints, [0, n]


RANGE_PAIRS = lambda k: [(3, 5), (0, 0), ((1 << k) - 1, 0), ((1 << k) - 1, 1), (R - 1, 2), (R - 1, 0)]   # noqa: E731


def nonzero(log_n):
    """x != 0.  inv = INV0(x); row 0 (driven): p = x * inv; row 1 (q_o = 0): p - 1 = 0.  (n, q, perm, hints, input cells)"""
    n = 1 << log_n
    q = _zero_q(n)
    q["q_m"][0] = q["q_o"][0] = 1
    q["q_l"][1], q["q_c"][1] = 1, R - 1
    return n, q, _perm_of(n, [[2 * n, 1]]), [(INV0, n, 0, 0, 0)], [0]


def hint_chain(log_n, shift=3, width=40):
    """a hint that reads a hint: inv = INV0(x) at b_0, bits = BITS(inv) at a_1, and row 2: c = inv + bits"""
    n = 1 << log_n
    q = _zero_q(n)
    q["q_l"][2] = q["q_r"][2] = q["q_o"][2] = 1
    return n, q, _perm_of(n, [[n, 2], [1, n + 2]]), [(INV0, n, 0, 0, 0), (BITS, 1, n, shift, width)], [0]


BIT_WINDOWS = [(0, 1), (0, 64), (1, 64), (29, 2), (30, 30), (31, 2), (60, 8), (63, 2), (127, 3), (191, 64), (250, 64), (254, 1)]


def bit_windows(log_n, windows=BIT_WINDOWS):
    """every window of one input (cell 0): hint i writes the a cell of row 1 + i"""
    n = 1 << log_n
    assert len(windows) + 1 <= n - 3
    return n, _zero_q(n), list(range(3 * n)), [(BITS, 1 + i, 0, s, w) for i, (s, w) in enumerate(windows)], [0]


def stacked(log_n, seed, shape, inputs=5):
    """a circuit built level by level: shape[l] = (rows, hints) of level l + 1.  A row's b operand and a hint's source are
    outputs of the level before (inputs at the first level): the first rows of a level read the hints of the level before, so
    every hint but the last level's is read.  Each hint writes the a cell of an otherwise empty row of its own.  Selectors are
    uniform non-zero on driven rows; hints alternate INV0 and BITS with seeded windows.  The last input is never assigned (it reads
    0, and the first hint of the first level, an INV0, reads it).  Row order is shuffled.
    Returns a dict: n, q, perm, hints, assigned, shape."""
    rng = random.Random(seed)
    n = 1 << log_n
    g = n - 3
    assert sum(r + h for r, h in shape) <= g
    pos = list(range(g))
    rng.shuffle(pos)
    q = _zero_q(n)
    classes = [[] for _ in range(inputs)]          # variable -> its cells
    anchor = {}                                    # variable -> a cell that holds it whoever reads it (a hint's src)
    pool, prev, hints, row = list(range(inputs)), list(range(inputs)), [], 0
    hint_prev = []
    for l, (rows, nh) in enumerate(shape):
        outs, must = [], list(hint_prev)
        for i in range(rows):
            j = pos[row]
            row += 1
            va, vb = rng.choice(pool), must.pop() if must else rng.choice(prev)
            classes[va].append(j)
            classes[vb].append(n + j)
            for name in W.SELECTORS:
                q[name][j] = rng.randrange(1, R)
            anchor[len(classes)] = 2 * n + j
            outs.append(len(classes))
            classes.append([2 * n + j])
        hint_prev = []
        for i in range(nh):
            j = pos[row]
            row += 1
            v = inputs - 1 if l == 0 and i == 0 else rng.choice(prev)
            if v not in anchor:                     # an input: any cell of it, or this row's b cell if nobody has read it yet
                if not classes[v]:
                    classes[v].append(n + j)
                anchor[v] = classes[v][0]
            kind = INV0 if len(hints) % 2 == 0 else BITS
            shift = rng.randrange(0, 255)
            hints.append((kind, j, anchor[v], shift if kind == BITS else 0, rng.randrange(1, 65) if kind == BITS else 0))
            anchor[len(classes)] = j
            hint_prev.append(len(classes))
            classes.append([j])
        pool += outs + hint_prev
        prev = outs + hint_prev
    assigned = {classes[v][0]: rng.randrange(1, R) for v in range(inputs - 1) if classes[v]}
    assigned.update(S.blinding_cells(n))
    return {"n": n, "q": q, "perm": _perm_of(n, classes), "hints": hints, "assigned": assigned, "shape": list(shape)}


def hint_wall(log_n, seed, rows=1000, mixed=37, n_hints=3041, run=130, readers=300, inputs=6):
    """three wide levels around a level of thousands of hints.  Level 1: `rows` rows over the inputs.  Level 2: `mixed` rows over
    the outputs of level 1, then `n_hints` hints, each of an output of level 1: hint h < rows is a BITS of output h, so every
    output feeds one; the next `run` are INV0, the `run` after them BITS, the rest INV0 or BITS by a seeded coin; a BITS hint h
    takes the window BIT_WINDOWS[h mod 12].  Level 3: `readers` rows whose operands are hint values.  Each hint writes the a cell
    of an otherwise empty row of its own; selectors are uniform non-zero on driven rows; row order is shuffled.  Three sets of
    inputs: under the last one the output that hint `zero_hint` (an INV0 inside the run) reads is 0, by that row's q_c -- the row
    is `zero_row`, and a public value there would undo it.
    Returns a dict: n, q, perm, hints, assigned (three {cell: value}), zero_row, zero_hint."""
    rng = random.Random(seed)
    n = 1 << log_n
    g = n - 3
    assert rows + mixed + n_hints + readers <= g and rows + 2 * run <= n_hints
    pos = list(range(g))
    rng.shuffle(pos)
    q = _zero_q(n)
    classes = [[] for _ in range(inputs)]          # variable -> its cells; an output's first cell is its row's c cell
    ops, at = {}, iter(pos)

    def driven(va, vb):
        j = next(at)
        classes[va].append(j)
        classes[vb].append(n + j)
        for name in W.SELECTORS:
            q[name][j] = rng.randrange(1, R)
        ops[len(classes)] = (j, va, vb)
        classes.append([2 * n + j])
        return len(classes) - 1

    outs = [driven(rng.randrange(inputs), rng.randrange(inputs)) for _ in range(rows)]
    for _ in range(mixed):
        driven(rng.choice(outs), rng.choice(outs))
    zero_out, zero_hint = outs[rows // 2], rows + run // 2
    hints, hint_vars = [], []
    for h in range(n_hints):
        j = next(at)
        if h < rows:
            kind, v = BITS, outs[h]
        elif h < rows + run:
            kind, v = INV0, zero_out if h == zero_hint else rng.choice(outs)
        elif h < rows + 2 * run:
            kind, v = BITS, rng.choice(outs)
        else:
            kind, v = rng.choice((INV0, BITS)), rng.choice(outs)
        shift, width = BIT_WINDOWS[h % len(BIT_WINDOWS)] if kind == BITS else (0, 0)
        hints.append((kind, j, classes[v][0], shift, width))
        hint_vars.append(len(classes))
        classes.append([j])
    for _ in range(readers):
        driven(rng.choice(hint_vars), rng.choice(hint_vars))
    assert all(classes[v] for v in range(inputs))
    assigned = []
    for _ in range(3):
        assigned.append({classes[v][0]: rng.randrange(1, R) for v in range(inputs)})
        assigned[-1].update(S.blinding_cells(n))
    zero_row, va, vb = ops[zero_out]
    a, b = assigned[2][classes[va][0]], assigned[2][classes[vb][0]]
    q["q_c"][zero_row] = -(q["q_l"][zero_row] * a + q["q_r"][zero_row] * b + q["q_m"][zero_row] * a * b) % R
    return {"n": n, "q": q, "perm": _perm_of(n, classes), "hints": hints, "assigned": assigned, "zero_row": zero_row,
            "zero_hint": zero_hint}
