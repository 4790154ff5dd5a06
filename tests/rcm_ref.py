"""Test-side reference of spmvHipRcmCSR (include/spmvHip.h): the serial queue loop in plain Python (rcm_loop), a second,
independent level-synchronous implementation on numpy arrays (rcm_levels, which can also plant three faults), the
bandwidth of a pattern under a permutation, and the small pattern cases the two test files share."""
import numpy as np

import colour_ref as cr

MIN_DEGREE, PERIPHERAL = 0, 1
FAULTS = ("children_by_id", "largest_parent", "reverse_per_component")


def adjacency(M, IRP, JA):
    """adj(i) as sorted lists: the pattern of A + A^T, repeats once, no diagonal, column ids >= M skipped"""
    adj = [set() for _ in range(M)]
    for i in range(M):
        for p in range(int(IRP[i]), int(IRP[i + 1])):
            j = int(JA[p])
            if j == i or j >= M:
                continue
            adj[i].add(j)
            adj[j].add(i)
    return [sorted(a) for a in adj]


def _level_structure(adj, deg, r, unvisited):
    """(depth, the vertex of the last level of smallest (deg, id)) of the BFS from r inside `unvisited`"""
    seen = {r}
    level = [r]
    depth = 0
    while level:
        depth += 1
        last = level
        nxt = []
        for u in level:
            for j in adj[u]:
                if j in unvisited and j not in seen:
                    seen.add(j)
                    nxt.append(j)
        level = nxt
    return depth, min(last, key=lambda v: (deg[v], v))


def rcm_loop(M, IRP, JA, start=PERIPHERAL, max_passes=0, forward=False):
    """the loop of include/spmvHip.h, word for word.  Returns (perm, info): info has components, levels, startBfs,
    maxFrontier as spmvRcmInfo defines them."""
    adj = adjacency(M, IRP, JA)
    deg = [len(a) for a in adj]
    max_passes = max_passes or 8
    by_deg = sorted(range(M), key=lambda v: (deg[v], v))
    cursor = 0
    unvisited = set(range(M))
    order = []
    info = dict(components=0, levels=0, startBfs=0, maxFrontier=0)
    while unvisited:
        while by_deg[cursor] not in unvisited:
            cursor += 1
        r = by_deg[cursor]
        info["components"] += 1
        if start == PERIPHERAL:
            depth, v = _level_structure(adj, deg, r, unvisited)
            n = 1
            while n <= max_passes:
                if v == r:
                    break
                depth_v, v_next = _level_structure(adj, deg, v, unvisited)
                n += 1
                if depth_v > depth:
                    r, depth, v = v, depth_v, v_next
                else:
                    break
            info["startBfs"] += n
        queue, head = [r], 0
        unvisited.discard(r)
        level_of = {r: 0}
        while head < len(queue):
            u = queue[head]
            head += 1
            order.append(u)
            for j in sorted((j for j in adj[u] if j in unvisited), key=lambda j: (deg[j], j)):
                unvisited.discard(j)
                level_of[j] = level_of[u] + 1
                queue.append(j)
        sizes = np.bincount(np.array([level_of[u] for u in queue]))
        info["levels"] += sizes.size
        info["maxFrontier"] = max(info["maxFrontier"], int(sizes.max()))
    perm = order if forward else order[::-1]
    return np.array(perm, dtype=np.uint32).reshape(M), info


def _edges(M, IRP, JA):
    """the deduplicated directed edges (a, b) of A + A^T without the diagonal, and the degrees"""
    IRP, JA = np.asarray(IRP, dtype=np.int64), np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    keep = (JA != rows) & (JA < M)
    key = np.unique(np.concatenate([rows[keep] * M + JA[keep], JA[keep] * M + rows[keep]])) if M else np.zeros(0, np.int64)
    a, b = (key // M, key % M) if M else (key, key)
    return a, b, np.bincount(a, minlength=M).astype(np.int64)


def rcm_levels(M, IRP, JA, start=PERIPHERAL, max_passes=0, forward=False, fault=None):
    """the level-synchronous form: level l + 1 = the unvisited vertices adjacent to level l, each with parent = the smallest
    position of a level-l neighbour, laid out in ascending (parent, deg, id).  fault plants one of FAULTS."""
    a, b, deg = _edges(M, IRP, JA)
    ptr = np.zeros(M + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(deg)
    max_passes = max_passes or 8
    by_deg = np.lexsort((np.arange(M), deg))
    rank = np.empty(M, dtype=np.int64)
    rank[by_deg] = np.arange(M)
    pos = np.full(M, -1, dtype=np.int64)                       # the place in `order` of a visited vertex
    order = np.empty(M, dtype=np.int64)
    done = 0

    def neighbours(front):
        """(the neighbour, the place in `front` of the vertex it is a neighbour of), for every edge out of front"""
        cnt = ptr[front + 1] - ptr[front]
        src = np.repeat(np.arange(front.size), cnt)
        idx = np.repeat(ptr[front] - np.cumsum(cnt) + cnt, cnt) + np.arange(int(cnt.sum()))
        return b[idx], src

    def search(r):
        seen = np.zeros(M, dtype=bool)
        seen[r] = True
        front, depth = np.array([r]), 0
        while front.size:
            depth, last = depth + 1, front
            w, _ = neighbours(front)
            w = np.unique(w[~seen[w] & (pos[w] < 0)])
            seen[w] = True
            front = w
        return depth, int(by_deg[rank[last].min()])

    cursor, info, parts = 0, dict(components=0, levels=0, startBfs=0, maxFrontier=0), []
    while done < M:
        while pos[by_deg[cursor]] >= 0:
            cursor += 1
        r = int(by_deg[cursor])
        info["components"] += 1
        if start == PERIPHERAL:
            depth, v = search(r)
            n = 1
            while n <= max_passes and v != r:
                depth_v, v_next = search(v)
                n += 1
                if depth_v <= depth:
                    break
                r, depth, v = v, depth_v, v_next
            info["startBfs"] += n
        first = done
        order[done], pos[r] = r, done
        lo, done = done, done + 1
        while True:
            info["levels"] += 1
            info["maxFrontier"] = max(info["maxFrontier"], done - lo)
            w, src = neighbours(order[lo:done])
            new = pos[w] < 0
            w, src = w[new], src[new]
            if not w.size:
                break
            parent = np.full(M, -1 if fault == "largest_parent" else M, dtype=np.int64)
            (np.maximum if fault == "largest_parent" else np.minimum).at(parent, w, src)
            w = np.unique(w)
            keys = (w, parent[w]) if fault == "children_by_id" else (w, deg[w], parent[w])
            w = w[np.lexsort(keys)]
            order[done:done + w.size] = w
            pos[w] = done + np.arange(w.size)
            lo, done = done, done + w.size
        parts.append(order[first:done].copy())
    if fault == "reverse_per_component":
        perm = np.concatenate([p[::-1] for p in parts]) if parts else order
    else:
        perm = order if forward else order[::-1]
    return perm.astype(np.uint32).reshape(M), info


def bandwidth(M, IRP, JA, perm=None):
    """max |new(i) - new(j)| over the stored entries with both ids < M (perm None: A's own numbering)"""
    IRP, JA = np.asarray(IRP, dtype=np.int64), np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    keep = JA < M
    inv = np.arange(M, dtype=np.int64)
    if perm is not None:
        inv[np.asarray(perm, dtype=np.int64)] = np.arange(M)
    d = np.abs(inv[rows[keep]] - inv[JA[keep]])
    return int(d.max()) if d.size else 0


# ------------------------------------------------------------------------------------------------- patterns
def from_edges(M, a, b, seed=None):
    """the symmetric pattern of the undirected edges (a, b) with a full diagonal, rows sorted; seed: the vertices renamed by
    a seeded random permutation first"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if seed is not None:
        name = np.random.default_rng(seed).permutation(M)
        a, b = name[a], name[b]
    key = np.unique(np.concatenate([a * M + b, b * M + a, np.arange(M) * (M + 1)]))
    return (M,) + cr.csr_of(M, key // M, key % M)


def path(M, seed=None):
    return from_edges(M, np.arange(M - 1), np.arange(1, M), seed)


def grid(nx, ny, nz=1, seed=None):
    ids = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = ids % nx, ids // nx % ny, ids // (nx * ny)
    a = np.concatenate([ids[x < nx - 1], ids[y < ny - 1], ids[z < nz - 1]])
    b = np.concatenate([ids[x < nx - 1] + 1, ids[y < ny - 1] + nx, ids[z < nz - 1] + nx * ny])
    return from_edges(ids.size, a, b, seed)


def star(leaves):
    return from_edges(leaves + 1, np.zeros(leaves, dtype=np.int64), 1 + np.arange(leaves), seed=5)


def three_components(seed=21):
    """a 9 x 7 grid, a path of 40, a cycle of 12 and 6 isolated vertices, renamed together"""
    ga, gb = _edge_list(grid(9, 7))
    M = 63 + 40 + 12 + 6
    a = np.concatenate([ga, 63 + np.arange(39), 103 + np.arange(12)])
    b = np.concatenate([gb, 63 + np.arange(1, 40), 103 + (np.arange(12) + 1) % 12])
    return from_edges(M, a, b, seed)


def _edge_list(case):
    M, IRP, JA = case
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP.astype(np.int64)))
    up = JA.astype(np.int64) > rows
    return rows[up], JA.astype(np.int64)[up]


def random_graph(M, seed):
    """about 4 neighbours each"""
    rng = np.random.default_rng(seed)
    return from_edges(M, rng.integers(0, M, 2 * M), rng.integers(0, M, 2 * M))


def small_cases():
    """name -> (M, IRP, JA): the colouring's small patterns and the ones the ordering adds"""
    out = dict(cr.small_cases())
    out["path3000"] = path(3000, seed=31)
    # (the names decide which neighbour of the start corner comes first, and with it the direction in which the levels are
    # laid out: 30 or 31 on the 2-D grid, 74 to 77 on the 3-D one.  These two seeds give the 30 and the 75 that
    # tests/test_rcm_abi.py pins.)
    out["grid40x30"] = grid(40, 30, seed=38)
    out["grid12x10x8"] = grid(12, 10, 8, seed=34)
    out["three_components"] = three_components()
    out["star1500"] = star(1500)
    out["random2000"] = random_graph(2000, 34)
    return out


CONFIGS = ((PERIPHERAL, False), (PERIPHERAL, True), (MIN_DEGREE, False), (MIN_DEGREE, True))     # (start, forward)
