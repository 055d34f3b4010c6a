"""ORBextractor::DistributeOctTree (reference ORBextractor.cc:544-750) restated as rounds of independent steps, in plain Python over
lists: what the device quadtree (sivo_amd/csrc/orb_quadtree_math.hpp) computes, written the way the formulation is stated and not
the way the kernel stores it (cells carry their candidates' indices here; the kernel keeps one list position per candidate).

A full round: let p1 .. pm be the non-leaf cells in list order.  Every one splits on its own; the new list is the non-empty children
of pm in the order SE, SW, NE, NW, then those of pm-1, ... p1, then the old leaves in their order; `grown` is the children with more
than one candidate in creation order (p1's NW, NE, SW, SE, then p2's ...).  A pass of the close-to-target phase: sort `grown` by
(size, creation order) descending, split all of them speculatively, scan (non-empty children - 1) on top of the count, stop at the
first place J that reaches the target (the last one if none does); places 0 .. J are split, the children of J come first.

distribute() also reports what it did: the full rounds, the passes of the close-to-target phase, the stop place and the length of
`grown` of every pass, and whether a pass met equal sizes in `grown` — the scenes of tests/orb_quadtree_cases.py assert the branch they
are named for through these."""
import math

import numpy as np


def roots_of(width, height):
    """n_ini = std::round((float)W / H) (halves away from zero), h_x = (float)W / n_ini — in float, as the reference."""
    ratio = np.float32(width) / np.float32(height)
    n_ini = int(math.floor(float(ratio) + 0.5))
    h_x = np.float32(width) / np.float32(n_ini) if n_ini > 0 else np.float32(0)
    return n_ini, h_x


def _split(box, idx, xs, ys):
    x0, y0, x1, y1 = box
    mx, my = x0 + ((x1 - x0 + 1) >> 1), y0 + ((y1 - y0 + 1) >> 1)           # ceil((float)d / 2) == (d + 1) >> 1
    boxes = [(x0, y0, mx, my), (mx, y0, x1, my), (x0, my, mx, y1), (mx, my, x1, y1)]      # NW, NE, SW, SE
    parts = [[], [], [], []]
    for i in idx:
        parts[(0 if xs[i] < mx else 1) + (0 if ys[i] < my else 2)].append(i)
    return [(boxes[q], parts[q]) for q in range(4)]


def distribute(keys, min_x, max_x, min_y, max_y, target, later_wins_ties=True):
    """The kept keys (a copy of the input's rows, in list order) and the report.  later_wins_ties=False breaks equal sizes in `grown`
    the other way (the earlier-created cell first): NOT what the library does; the tie scene shows that it matters."""
    xs = [int(v) for v in keys["x"]]; ys = [int(v) for v in keys["y"]]; rs = [int(v) for v in keys["response"]]
    report = dict(rounds=0, passes=0, stops=[], grown=[], tie_in_grown=False, ended_unchanged=False, n_ini=0)
    if len(keys) == 0:
        return keys[:0].copy(), report
    width, height = max_x - min_x, max_y - min_y
    n_ini, h_x = roots_of(width, height)
    report["n_ini"] = n_ini
    roots = [((int(h_x * np.float32(i)), 0, int(h_x * np.float32(i + 1)), height), []) for i in range(n_ini)]
    for i, x in enumerate(xs):
        roots[int(np.float32(x) / h_x)][1].append(i)         # NOT the root whose box holds x
    cells = [c for c in roots if c[1]]
    grown, full = [], True
    while True:
        before = len(cells)
        if full:
            report["rounds"] += 1
            parents = [c for c in cells if len(c[1]) > 1]
            leaves = [c for c in cells if len(c[1]) == 1]
            kids = [_split(c[0], c[1], xs, ys) for c in parents]
            front = [k[q] for k in reversed(kids) for q in (3, 2, 1, 0) if k[q][1]]
            cells = front + leaves
            grown = [k[q] for k in kids for q in range(4) if len(k[q][1]) > 1]
            if len(cells) >= target or len(cells) == before:
                report["ended_unchanged"] = len(cells) < target
                break
            if len(cells) + 3 * len(grown) > target:
                full = False
            continue
        report["passes"] += 1
        sizes = [len(c[1]) for c in grown]
        report["tie_in_grown"] |= len(set(sizes)) < len(sizes)
        order = sorted(range(len(grown)), key=lambda e: (sizes[e], e if later_wins_ties else -e), reverse=True)
        kids = [_split(grown[e][0], grown[e][1], xs, ys) for e in order]
        running, stop = before, len(order) - 1
        for place, k in enumerate(kids):                      # the inclusive scan; the first place that reaches the target
            running += sum(1 for q in range(4) if k[q][1]) - 1
            if running >= target:
                stop = place
                break
        report["stops"].append(stop); report["grown"].append(len(order))
        split_now = {id(grown[e]) for e in order[:stop + 1]}
        front = [kids[place][q] for place in range(stop, -1, -1) for q in (3, 2, 1, 0) if kids[place][q][1]]
        cells = front + [c for c in cells if id(c) not in split_now]
        grown = [kids[place][q] for place in range(stop + 1) for q in range(4) if len(kids[place][q][1]) > 1]
        if len(cells) >= target or len(cells) == before:
            report["ended_unchanged"] = len(cells) < target
            break
    best = [max(c[1], key=lambda i: (rs[i], -i)) for c in cells]          # greatest response, then smallest index
    return keys[best].copy(), report
