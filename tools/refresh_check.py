"""
Imputation after a refresh against imputation on a fresh upload of the same numbers, in a process of its own (switches such
as GRIM_NO_SMALL are read once per process):

    python tools/refresh_check.py cau_full

refreshes the CAU graph on the device with seeded counts, imputes a fully typed input on it, uploads a second graph that
holds the CPU twin's frequencies and imputes the same input there.  Prints one JSON line; exit status 0 when the six output
texts are equal byte for byte and differ from those before the refresh.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import harness  # noqa: E402
import refresh_synth as rs  # noqa: E402
import synth  # noqa: E402


def refreshed_pair(imp, seed):
    """refreshes imp's graph with seeded counts -> (statistics, an Imputation on a fresh graph with the twin's frequencies)"""
    from grim import _native as nat
    from grim.em import refresh_freq_arrays

    g = imp.netGraph
    keys, pops, counts = rs.random_counts(g.arrays, seed=seed, absent=0.3)
    want, _ = refresh_freq_arrays(g.arrays, keys, pops, counts)
    stats = g.refresh(nat.default_context(imp.device), (keys, pops, counts))
    assert g.arrays["freq"].tobytes() == want.tobytes(), "the refreshed frequencies differ from the twin's"
    return stats, rs.with_freq(imp, want)


def main(argv):
    case = argv[1] if len(argv) > 1 else "cau_full"
    if case != "cau_full":
        raise SystemExit("unknown case %r" % case)
    rows = synth.read_freqs(synth.CAU_FREQS)
    lines = synth.SubjectGen(rows, 123).full(64)
    imp = rs.own_imputation("cau", harness.base_conf(["CAU"]), tag="refresh_check")
    before = imp.impute_lines(lines, imp.config)
    stats, fresh = refreshed_pair(imp, seed=11)
    after = imp.impute_lines(lines, imp.config)
    want = fresh.impute_lines(lines, fresh.config)
    same = all(after[k] == want[k] for k in want)
    changed = any(after[k] != before[k] for k in want)
    print(json.dumps({"case": case, "no_small": os.environ.get("GRIM_NO_SMALL", ""), "same": same, "changed": changed,
                      "subjects": imp.last_stats.get("n", 0), "rows_after": after["umug"].count("\n"), "zero_full": stats["zero_full"],
                      "differs": [k for k in want if after[k] != want[k]]}))
    return 0 if same and changed else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
