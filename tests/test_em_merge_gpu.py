"""The merge doors of the M-step accumulator (csrc/grim_em.h em_merge_kernel / em_merge_records_kernel through
EmAccumulator.merge / merge_records) against the CPU twin (grim.em.merge_tables, fold_chunk_tables), bit for bit: table
growth inside a merge, populations up to mask bit 63, sizes around the 256-lane block, key sets that are disjoint, identical and
half shared, the order of merges, both doors mixed with each other and with accumulate, every refusal, and m_step_chunked
on a real input against the record twin per chunk."""
import numpy as np
import pytest

import harness
import test_em_gpu as shapes

pytestmark = pytest.mark.gpu

N_ALLELES = shapes.N_ALLELES
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]
MERGE_KEPT = ("subjects_used", "skipped_plan_c", "contributions")


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


def _key(j):
    return shapes._key([1 + j % 3000, 1 + j // 3000, 3, 4, 5])


def table(n, P, seed=0, first_key=0):
    """n entries in export order: keys numbered from `first_key`, key j in the populations (63 + j + t) mod P for t < min(P, 3)
    (key 0 of 64 populations sets mask bit 63); counts of mixed magnitude, every seventh +0.0"""
    per = min(P, 3)
    ent = {}
    for i in range(n):
        j, t = i // per, i % per
        x = [0.1, 0.2, 0.3][(i + seed) % 3] * 10.0 ** -((i + 2 * seed) % 5)
        ent[(_key(first_key + j), (63 + first_key + j + t) % P)] = 0.0 if (i + seed) % 7 == 3 else x
    order = sorted(ent)
    return (np.array([k for k, _ in order], dtype=np.uint64), np.array([p for _, p in order], dtype=np.uint32),
            np.array([ent[at] for at in order], dtype=np.float64))


def n_keys(t):
    return len(set(t[0].tolist()))


def _hex(t):
    return list(zip(t[0].tolist(), t[1].tolist(), [float(x).hex() for x in t[2].tolist()]))


def _acc(ctx, P, first_capacity=64):
    from grim import _native as nat

    return nat.EmAccumulator(ctx, N_ALLELES, P, first_capacity)


@pytest.mark.parametrize("overlap", ["disjoint", "identical", "half"])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_both_doors_equal_the_twin(ctx, P, overlap):
    """B merged into an accumulator that holds A, for every size of both: through the records door, and through the table
    door from an accumulator that holds B alone.  first_capacity 64: more than 32 keys force the table to grow inside a merge."""
    from grim.em import fold_chunk_tables

    for n in SIZES:
        A = table(n, P, seed=1)
        first = {"disjoint": n_keys(A), "identical": 0, "half": n_keys(A) // 2}[overlap]
        for m in sorted({n, SIZES[(SIZES.index(n) + 3) % len(SIZES)]}):
            B = table(m, P, seed=2, first_key=first)
            want = fold_chunk_tables([A, B], P, N_ALLELES)
            if n and m:
                shared = len(set(zip(A[0].tolist(), A[1].tolist())) & set(zip(B[0].tolist(), B[1].tolist())))
                assert (shared == 0) == (overlap == "disjoint")
            if P == 64 and n:
                assert 63 in want[1].tolist()
            dst, src, both = _acc(ctx, P), _acc(ctx, P), _acc(ctx, P)
            try:
                dst.merge_records(*A)
                assert _hex(dst.export()) == _hex(A) and dst.entries() == n
                src.merge_records(*B)
                dst.merge(src)
                assert _hex(dst.export()) == _hex(want), "table door: %d into %d" % (m, n)
                assert dst.entries() == len(want[0])
                assert _hex(src.export()) == _hex(B)  # the source is not changed
                both.merge_records(*A)
                both.merge_records(*B)
                assert _hex(both.export()) == _hex(want), "records door: %d into %d" % (m, n)
                if n_keys(want) > 32:
                    assert dst.stats()["rehashes"] > 0 and both.stats()["rehashes"] > 0
                assert (dst.merge_ms() > 0.0) == (m > 0)
                assert dst.kernel_ms() == 0.0 and {k: dst.stats()[k] for k in MERGE_KEPT} == dict.fromkeys(MERGE_KEPT, 0)
            finally:
                dst.close(), src.close(), both.close()


def test_a_chain_of_three_merges(ctx):
    from grim.em import fold_chunk_tables

    P = 3
    tables = [table(257, P, seed=1), table(300, P, seed=2, first_key=40), table(65, P, seed=3, first_key=20)]
    want = fold_chunk_tables(tables, P, N_ALLELES)
    master, by_records = _acc(ctx, P), _acc(ctx, P)
    try:
        for t in tables:
            part = _acc(ctx, P, 1 << 10)
            try:
                part.merge_records(*t)
                master.merge(part)
            finally:
                part.close()
            by_records.merge_records(*t)
        assert _hex(master.export()) == _hex(want) == _hex(by_records.export())
    finally:
        master.close(), by_records.close()


def test_order_witness_on_the_device(ctx):
    """1.0, 2^-53, 2^-53 merged in this order is exactly 1.0; 1.0 + (2^-53 + 2^-53) would be 1 + 2^-52, and so is the reverse
    order: the device adds one table at a time to what it holds, in the caller's order"""
    k, t = np.array([_key(5)], dtype=np.uint64), 2.0 ** -53
    pop = np.array([1], dtype=np.uint32)
    for door in ("records", "table"):
        for values, want in (((1.0, t, t), 1.0), ((t, t, 1.0), 1.0 + 2.0 ** -52)):
            master = _acc(ctx, 3)
            try:
                for x in values:
                    if door == "records":
                        master.merge_records(k, pop, np.array([x]))
                    else:
                        part = _acc(ctx, 3)
                        try:
                            part.merge_records(k, pop, np.array([x]))
                            master.merge(part)
                        finally:
                            part.close()
                assert _hex(master.export()) == [(int(k[0]), 1, float(want).hex())], (door, values)
            finally:
                master.close()


def test_merges_mix_with_accumulate(ctx):
    """a merge into an accumulator that already took records, and records accumulated after a merge: the twin carries one
    dict through fold_records and merge_tables in the same order.  A merge moves neither the batch statistics nor the spill"""
    from grim.em import fold_records, merge_tables, table_arrays

    P = shapes.N_POPS
    res, rows = shapes.em_records(shapes.shape_subjects(1, P, [1, 63, 65]))
    res2, rows2 = shapes.em_records(shapes.shape_subjects(2, P, [2, 64])[5:])
    keys = fold_records(res, rows, N_ALLELES, P)[0]
    # a table on keys the records name (every third) and on others
    T = table(200, P, seed=4)
    mine = keys[::3][:60]
    T = table_arrays(merge_tables({(int(k), 1): 0.25 for k in mine.tolist()}, *T))
    carry = {}
    acc, src = _acc(ctx, P), _acc(ctx, P, 1 << 12)
    try:
        src.merge_records(*T)
        acc.accumulate_records(res, rows)
        w1 = fold_records(res, rows, N_ALLELES, P, batch=0, carry=carry)
        before = (shapes._got(acc)[3:], acc.last_unsupported(), acc.kernel_ms())
        assert len(before[0][0]) > 0 and acc.kernel_ms() > 0.0
        acc.merge(src)
        merge_tables(carry, *T, n_pops=P, n_alleles=N_ALLELES)
        assert _hex(acc.export()) == _hex(table_arrays(carry))
        assert (shapes._got(acc)[3:], acc.last_unsupported(), acc.kernel_ms()) == before
        acc.accumulate_records(res2, rows2)
        w2 = fold_records(res2, rows2, N_ALLELES, P, batch=1, carry=carry)  # the merge did not count as a batch
        assert _hex(acc.export()) == _hex(w2[:3])
        assert [tuple(x) for x in acc.spill().tolist()] == [tuple(x) for x in w1[3].tolist()] + [tuple(x) for x in w2[3].tolist()]
        acc.merge_records(*T)
        merge_tables(carry, *T, n_pops=P, n_alleles=N_ALLELES)
        assert _hex(acc.export()) == _hex(table_arrays(carry))
        assert acc.stats()["contributions"] == w1[4]["contributions"] + w2[4]["contributions"]
    finally:
        acc.close(), src.close()


def test_refusals_change_nothing(ctx):
    from grim import _native as nat

    L = nat._em_lib()
    P = 3
    A = table(100, P, seed=1)
    res, rows = shapes.em_records(shapes.shape_subjects(1, P, [1, 65]))
    acc = _acc(ctx, P, 1 << 10)
    other_ctx = nat.Context(ctx.device)
    others = {"the source is the destination": acc,
              "another context": nat.EmAccumulator(other_ctx, N_ALLELES, P, 64),
              "another number of populations": _acc(ctx, P + 1),
              "another n_alleles": nat.EmAccumulator(ctx, N_ALLELES[:4] + [N_ALLELES[4] + 1], P, 64)}
    try:
        acc.accumulate_records(res, rows)
        acc.merge_records(*A)
        assert acc.merge_ms() > 0.0
        before = (_hex(acc.export()), shapes._got(acc)[3:], acc.stats(), acc.entries(), acc.kernel_ms())
        assert len(before[1][0]) > 0

        def untouched(text):
            assert text in ctx.error(), ctx.error()
            assert (_hex(acc.export()), shapes._got(acc)[3:], acc.stats(), acc.entries(), acc.kernel_ms()) == before
            assert acc.merge_ms() == 0.0

        for text, src in others.items():
            if src is not acc:
                src.merge_records(*table(5, P, seed=3))  # something to merge, were it not refused
            assert L.grim_em_merge(acc.h, src.h) == -3
            untouched("grim_em_merge: ")
            untouched(text)
            acc.merge_records(*table(0, P))  # a merge of nothing is no refusal, and changes nothing either
            with pytest.raises(nat.NativeError):
                acc.merge(src)

        def refused(k, p, c, text, n=None):
            k, p, c = np.array(k, dtype=np.uint64), np.array(p, dtype=np.uint32), np.array(c, dtype=np.float64)
            ptr = lambda a: nat._ptr(a) if a is not None else None
            assert L.grim_em_merge_records(acc.h, ptr(k), ptr(p), ptr(c), len(k) if n is None else n) == -3
            untouched("grim_em_merge_records: ")
            untouched(text)

        k1, k2 = _key(1), _key(2)
        for missing in range(3):
            args = [np.array([k1], dtype=np.uint64), np.array([0], dtype=np.uint32), np.array([1.0])]
            args[missing] = None
            assert L.grim_em_merge_records(acc.h, *[nat._ptr(a) if a is not None else None for a in args], 1) == -3
            untouched("a null array with n > 0")
        refused([k1], [P], [1.0], "a population at or above the accumulator's number of populations")
        refused([k1, k2], [0, P + 60], [1.0, 1.0], "a population at or above")
        refused([k1 | 1 << 60], [0], [1.0], "a key with a bit at or above GRIM_KEY_GRAPH_ORDER")
        refused([shapes._key([N_ALLELES[0] + 1, 1, 1, 1, 1])], [0], [1.0], "a key with a field above n_alleles")
        refused([shapes._key([1, 1, 1, 1, 4095])], [0], [1.0], "a key with a field above n_alleles")
        refused([k2, k1], [0, 0], [1.0, 1.0], "not strictly ascending in (key, pop)")
        refused([k1, k1], [1, 1], [1.0, 1.0], "not strictly ascending in (key, pop)")
        refused([k1, k1], [2, 1], [1.0, 1.0], "not strictly ascending in (key, pop)")
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            refused([k1, k2], [0, 0], [1.0, bad], "a count that is negative, NaN or infinite")
        with pytest.raises(ValueError):
            acc.merge_records([k1, k2], [0], [1.0, 1.0])
        # a field AT n_alleles is a dictionary allele, and the accumulator works after the refusals
        top = (np.array([shapes._key([N_ALLELES[0], 1, 1, 1, 1])], dtype=np.uint64), np.array([P - 1], dtype=np.uint32), np.array([2.0]))
        acc.merge_records(*top)
        assert acc.entries() == before[3] + 1 and acc.merge_ms() > 0.0
    finally:
        for a in others.values():
            a.close()
        acc.close()
        other_ctx.close()


# ---- a real input: m_step_chunked against the record twin per chunk ------------------------------------------------------------
@pytest.fixture(scope="module")
def pop4_mixed():
    gname, conf, lines, _, _, _ = harness.golden("pop4_mixed")
    _, _, imp = harness.run_product(gname, conf, lines, tag="em_merge_mixed", em_mr=True, on_unsupported="skip", quiet=True)
    return lines, imp, bool(conf.get("_em"))


def _counts_hex(counts):
    return {pop: {hap: float(c).hex() for hap, c in d.items()} for pop, d in counts.items()}


def test_m_step_chunked_equals_the_twin_fold(pop4_mixed):
    from grim.blocks import Blocks
    from grim.em import fold_chunk_tables, fold_records, m_step_chunked

    lines, imp, em = pop4_mixed
    g = imp.netGraph
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    P = len(imp.populations)
    assert 250 <= len(lines) <= 350
    shared = Blocks(imp, imp.config, None, True, em, output_haplotypes=True)
    tables, sums = [], dict.fromkeys(MERGE_KEPT, 0)
    for lo in range(0, len(lines), 50):
        block = shared.block(lines[lo:lo + 50], lo)
        try:
            out = fold_records(*block.records(), n_alleles, P)
        finally:
            block.close()
        tables.append(out[:3])
        for k in sums:
            sums[k] += out[4][k]
    want = fold_chunk_tables(tables, P, n_alleles)
    assert len(want[0]) > 200 and len(want[0]) < sum(len(t[0]) for t in tables)  # haplotypes recur across the chunks
    counts, stats, got = m_step_chunked(imp, lines, imp.config, 50, em=em)
    assert _hex(got) == _hex(want)
    assert {k: stats[k] for k in sums} == sums and stats["chunks"] == len(tables) == 6 and stats["entries"] == len(want[0])
    assert stats["merge_ms"] > 0.0 and stats["kernel_ms"] > 0.0
    named = {}
    for k, p, c in zip(*[a.tolist() for a in want]):
        named.setdefault(imp.populations[p], {})[g.key_to_name(k)] = float(c).hex()
    got_named = _counts_hex(counts)
    assert all(got_named[pop][hap] == c for pop, d in named.items() for hap, c in d.items())
    assert sum(len(d) for d in got_named.values()) >= sum(len(d) for d in named.values())
    # the block cuts inside a chunk do not show
    counts7, _, got7 = m_step_chunked(imp, lines, imp.config, 50, block_lines=7, em=em)
    assert _hex(got7) == _hex(got) and _counts_hex(counts7) == got_named


def test_one_chunk_is_m_step_counts(pop4_mixed):
    from grim.em import m_step_chunked, m_step_counts

    lines, imp, em = pop4_mixed
    want, wstats = m_step_counts(imp, lines, imp.config, em=em)
    for chunk_lines in (len(lines), 1 << 20):
        counts, stats, table = m_step_chunked(imp, lines, imp.config, chunk_lines, em=em)
        assert _counts_hex(counts) == _counts_hex(want)
        assert stats["chunks"] == 1
        for k in MERGE_KEPT + ("entries", "spill", "blocks"):
            assert stats[k] == wstats[k], k
