"""The PARALLEL form of the duplicate-key check, restated on the host exactly as tsq_dupcheck_* computes it (DESIGN.md §5 "Duplicate
keys and REPLACE"): per stream the store match and the previous statement row of every key, the candidate of the equality test, added /
put flags, the removed stored rows.  tests/test_dupcheck_cpu.py holds it to the sequential model of tests/dupcheck_ref.py on random
statements; the GPU tests take the candidate arrays from here (the model has no such thing) after that."""
from tests import dupcheck_ref as R


def streams_of(shape, stored, rows):
    """per stream: (the statement rows' keys, None where the row does not take part; {key: handle} of the store's entries)"""
    out = []
    if shape.pk_col is not None:
        out.append(([r[shape.pk_col] for r in rows], {h: h for h, _ in stored}))
    for i in range(len(shape.uniques)):
        ks, ds = R.index_keys(shape, i, rows)
        sk, sd = R.index_keys(shape, i, [r for _, r in stored])
        out.append(([k if d else None for k, d in zip(ks, ds)], {k: h for k, d, (h, _) in zip(sk, sd, stored) if d}))
    return out


def prev_and_match(streams, n):
    prev = [[-1] * n for _ in streams]
    match = [[None] * n for _ in streams]
    for s, (keys, smap) in enumerate(streams):
        last = {}
        for r, k in enumerate(keys):
            if k is None:
                continue
            prev[s][r] = last.get(k, -1)
            last[k] = r
            match[s][r] = smap.get(k)
    return prev, match


def parallel_insert(shape, stored, rows):
    """-> None, or (row, stream, from_store, dup_handle or None, dup_row or None)"""
    streams = streams_of(shape, stored, rows)
    prev, match = prev_and_match(streams, len(rows))
    for r in range(len(rows)):
        for s, (keys, _) in enumerate(streams):
            if match[s][r] is not None:
                return (r, s, True, match[s][r], None)
            if prev[s][r] >= 0:
                return (r, s, False, None, keys.index(keys[r]))  # the FIRST row of the key's group
    return None


def parallel_replace(shape, stored, rows, rowid_base=0):
    n = len(rows)
    streams = streams_of(shape, stored, rows)
    prev, match = prev_and_match(streams, n)
    old = dict(stored)
    cand, equal = [], []
    for r in range(n):
        j = max([p[r] for p in prev], default=-1)
        c = None
        if j >= 0:
            c = ("b", j)
        else:
            for s in range(len(streams)):
                if match[s][r] is not None:
                    c = ("s", match[s][r])
                    break
        cand.append(c)
        equal.append(c is not None and R.equal_datums(rows[c[1]] if c[0] == "b" else old[c[1]], rows[r]))
    added = [not e for e in equal]
    removed_store = sorted({match[s][r] for r in range(n) if added[r] for s in range(len(streams)) if match[s][r] is not None})
    removed = [False] * n
    for keys, _ in streams:
        gmax = {}
        for r, k in enumerate(keys):
            if k is not None and added[r]:
                gmax[k] = r
        for r, k in enumerate(keys):
            if k is not None and added[r] and gmax[k] > r:
                removed[r] = True
    handles, c = [], 0
    for r in range(n):
        c += added[r]
        handles.append(rowid_base + c if added[r] else None)
    if shape.pk_col is not None:
        handles = [rows[r][shape.pk_col] if added[r] else None for r in range(n)]
    put = [added[r] and not removed[r] for r in range(n)]
    table = {h: tuple(r) for h, r in stored if h not in set(removed_store)}
    for r in range(n):
        if put[r]:
            table[handles[r]] = tuple(rows[r])
    return dict(cand=cand, equal=equal, added=added, put=put, handles=handles, removed_store=removed_store, n_removed_batch=sum(removed),
                affected=n + len(removed_store) + sum(removed), rowid_base=rowid_base + (sum(added) if shape.pk_col is None else 0), table=table)
