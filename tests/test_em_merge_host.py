"""The sharded M-step's host side (grim/em.py): the merge twin and the chunk-ordered fold against an independent dict fold,
every refusal of the merge doors, the fold over record cuts against the documented sums, and the order witness that a
re-associated fold fails.  No GPU."""
import numpy as np
import pytest

N_ALLELES = [4000] * 5
N_POPS = 4
ABITS = 12


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _table(entries):
    """{(key, pop): count} -> arrays in export order"""
    order = sorted(entries)
    return (np.array([k for k, _ in order], dtype=np.uint64), np.array([p for _, p in order], dtype=np.uint32),
            np.array([entries[at] for at in order], dtype=np.float64))


def _chunk(c, n=40, P=N_POPS):
    """chunk c's table: keys that overlap with the neighbouring chunks', counts of mixed magnitude, some +0.0"""
    out = {}
    for i in range(n):
        key = _key([1 + (i + 13 * c) % 57, 2 + i % 3, 3, 4, 5 + (i * c) % 2])
        x = [0.1, 0.2, 0.3][(i + c) % 3] * 10.0 ** -((i + 2 * c) % 7)
        out[(key, (i + c) % P)] = 0.0 if i % 17 == 3 else x
    return out


def _independent_fold(tables):
    """the contract written out once more: per entry, the chunks that hold it in ascending chunk number, ((a + b) + c)"""
    where = {}
    for c, (keys, pops, counts) in enumerate(tables):
        for k, p, x in zip(keys.tolist(), pops.tolist(), counts.tolist()):
            where.setdefault((k, p), []).append(x)
    out = {}
    for at, xs in where.items():
        s = xs[0]
        for x in xs[1:]:
            s = (s + x)
        out[at] = s
    return out


def _hex(table):
    keys, pops, counts = table
    return list(zip(keys.tolist(), pops.tolist(), [float(x).hex() for x in counts.tolist()]))


def test_fold_equals_independent_fold():
    from grim.em import fold_chunk_tables, merge_tables, table_arrays

    tables = [_table(_chunk(c)) for c in range(5)] + [_table({})]
    want = _independent_fold(tables)
    assert len(want) < sum(len(t[0]) for t in tables)  # keys do recur across chunks
    got = fold_chunk_tables(tables, N_POPS, N_ALLELES)
    assert _hex(got) == _hex(_table(want))
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    # the same through merge_tables with one carry; the carry is the dict it returns
    carry = {}
    for t in tables:
        assert merge_tables(carry, *t, n_pops=N_POPS, n_alleles=N_ALLELES) is carry
    assert _hex(table_arrays(carry)) == _hex(got)
    # one table alone comes back as it is, +0.0 counts included
    one = fold_chunk_tables(tables[:1])
    assert _hex(one) == _hex(tables[0]) and 0.0 in one[2].tolist()
    assert _hex(fold_chunk_tables([])) == []


def test_order_witness():
    """1.0, 2^-53, 2^-53 in chunk order is exactly 1.0 (each half-ulp add rounds back to even); 1.0 + (2^-53 + 2^-53) is
    1 + 2^-52: a fold that re-associates, or that takes the chunks in another order, does not pass"""
    from grim.em import fold_chunk_tables

    k, t = _key([1, 2, 3, 4, 5]), 2.0 ** -53
    tables = [_table({(k, 1): x}) for x in (1.0, t, t)]
    assert 1.0 + (t + t) == 1.0 + 2.0 ** -52 != 1.0
    assert (t + t) + 1.0 != 1.0
    assert _hex(fold_chunk_tables(tables)) == [(k, 1, (1.0).hex())]
    assert _hex(fold_chunk_tables(tables[::-1])) == [(k, 1, (1.0 + 2.0 ** -52).hex())]


def test_every_refusal_leaves_the_carry_alone():
    from grim.em import merge_tables

    k1, k2 = _key([1, 2, 3, 4, 5]), _key([2, 2, 3, 4, 5])
    good = ([k1, k1, k2], [0, 3, 1], [1.0, 0.0, 2.5])
    bad = {
        "null array": (None, [0], [1.0]),
        "different lengths": ([k1, k2], [0], [1.0, 2.0]),
        "at or above the accumulator's number of populations": ([k1], [N_POPS], [1.0]),
        "bit at or above": ([k1 | 1 << 60], [0], [1.0]),
        "field above n_alleles": ([_key([4001, 2, 3, 4, 5])], [0], [1.0]),
        "not strictly ascending": ([k2, k1], [0, 0], [1.0, 1.0]),
        "not strictly ascending ": ([k1, k1], [1, 1], [1.0, 1.0]),
        "not strictly ascending  ": ([k1, k1], [2, 1], [1.0, 1.0]),
        "negative, NaN or infinite": ([k1], [0], [-1.0]),
        "negative, NaN or infinite ": ([k1], [0], [float("nan")]),
        "negative, NaN or infinite  ": ([k1], [0], [float("inf")]),
    }
    carry = merge_tables({}, *good, n_pops=N_POPS, n_alleles=N_ALLELES)
    before = dict(carry)
    for why, (keys, pops, counts) in bad.items():
        for head in ((), good):  # the refused entry first, or behind good ones: nothing of the call is added
            if head and keys is not None and len(keys) == len(pops) == len(counts):
                args = ([_key([1, 1, 1, 1, 1])] + list(keys), [0] + list(pops), [1.0] + list(counts))
            else:
                args = (keys, pops, counts)
            with pytest.raises(ValueError) as refused:
                merge_tables(carry, *args, n_pops=N_POPS, n_alleles=N_ALLELES)
            assert why.strip() in str(refused.value)
            assert carry == before
    # a field AT n_alleles is a dictionary allele; the checks that need the accumulator's shape are off without it
    merge_tables(carry, [_key([4000, 2, 3, 4, 5])], [N_POPS - 1], [1.0], n_pops=N_POPS, n_alleles=N_ALLELES)
    merge_tables({}, [_key([4001, 2, 3, 4, 5])], [N_POPS], [1.0])


def test_fold_over_record_cuts():
    """fold_records per chunk of subjects, each with a fresh carry; the tables merged in order are the documented sums: per
    entry the chunk tables added left to right, and with one chunk the whole fold itself"""
    import test_em_gpu as shapes

    from grim.em import fold_chunk_tables, fold_records

    subs = shapes.shape_subjects(rounds=2, sizes=[1, 2, 63, 65])
    res, rows = shapes.em_records(subs)
    whole = fold_records(res, rows, shapes.N_ALLELES, shapes.N_POPS)
    assert len(whole[0]) > 500
    assert _hex(fold_chunk_tables([whole[:3]], shapes.N_POPS, shapes.N_ALLELES)) == _hex(whole[:3])
    for step in (1, 7, 20):
        tables, stats = [], dict.fromkeys(("subjects_used", "skipped_plan_c", "contributions"), 0)
        for lo in range(0, len(subs), step):
            out = fold_records(*shapes.em_records(subs[lo:lo + step]), shapes.N_ALLELES, shapes.N_POPS)
            tables.append(out[:3])
            for k in stats:
                stats[k] += out[4][k]
        got = fold_chunk_tables(tables, shapes.N_POPS, shapes.N_ALLELES)
        assert _hex(got) == _hex(_table(_independent_fold(tables))), "chunks of %d subjects" % step
        assert got[0].tolist() == whole[0].tolist() and got[1].tolist() == whole[1].tolist()
        assert stats == {k: whole[4][k] for k in stats}
        # the chunked sums are another association of the same terms: a sum of m positive terms is within
        # (m - 1) u (1 + O(m u)), u = 2^-53, relative of the exact sum whatever the association, and no entry has more than
        # m = 2 * rows terms; so two associations differ by at most 2.02 m u of either
        m = 2 * len(rows)
        assert np.all(np.abs(got[2] - whole[2]) <= 2.02 * m * 2.0 ** -53 * whole[2])


def test_input_chunks_cut_a_file_where_chunk_offsets_does(tmp_path):
    """a file and the list of its lines give the same chunks, whatever ends the lines; the first line of chunk c is c * chunk_lines"""
    from grim.em import input_chunks

    rows = ["D%d,A*01:01+A*02:01" % i for i in range(23)]
    for sep_cycle in (["\n"], ["\r\n"], ["\n", "\r\n", "\r"]):
        for tail in (True, False):
            data = "".join(r + sep_cycle[i % len(sep_cycle)] for i, r in enumerate(rows))
            if not tail:
                data = data[:-len(sep_cycle[(len(rows) - 1) % len(sep_cycle)])]
            p = tmp_path / "in.csv"
            p.write_bytes(data.encode())
            for chunk in (1, 5, 23, 100):
                want = [(lo, rows[lo:lo + chunk]) for lo in range(0, len(rows), chunk)]
                assert list(input_chunks(str(p), chunk)) == want
                assert list(input_chunks(p, chunk)) == want
                assert list(input_chunks([r + "\n" for r in rows], chunk)) == want
    p.write_bytes(b"")
    assert list(input_chunks(str(p), 4)) == [] == list(input_chunks([], 4))
