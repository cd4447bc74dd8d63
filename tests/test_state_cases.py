"""The state-independence cases cover the header: every C entry include/bmo.h declares is reached by a case of tests/state_cases.py or
is on its written exclusion list, and bmo_amd.abi allocates every buffer a C entry writes through its one helper `_out`, which
tests/test_state_independence_gpu.py swaps for a filler of sentinel words.  No device, no build: the cases are not run here."""
import ast
import os

import state_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = os.path.join(ROOT, "beamletoptics.jl_amd", "abi.py")


def test_every_entry_of_the_header_has_a_case_or_a_reason():
    declared = sc.header_entries()
    assert len(declared) >= 55 and "bmo_trace" in declared and "bmo_psf_poly_otf" in declared, sorted(declared)  # (the search finds them)
    covered = set().union(*(f.entries for f in sc.CASES))
    assert covered <= declared, "a case names an entry the header does not declare: %r" % sorted(covered - declared)
    assert set(sc.EXCLUDED) <= declared, "excluded, but not declared: %r" % sorted(set(sc.EXCLUDED) - declared)
    assert not covered & set(sc.EXCLUDED), "both covered and excluded: %r" % sorted(covered & set(sc.EXCLUDED))
    missing = declared - covered - set(sc.EXCLUDED)
    assert not missing, "entries of include/bmo.h without a state-independence case (tests/state_cases.py): %r" % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 10 for r in sc.EXCLUDED.values())


def test_cases_are_named_once_and_grouped():
    names = [f.name for f in sc.CASES]
    assert len(names) == len(set(names))
    assert {f.group for f in sc.CASES} == set(sc.GROUPS)
    assert all(f.entries for f in sc.CASES)


def test_the_row_counts_recycle_a_larger_block():
    """300 rows directly before 257: the pool hands a block out for a request if it is at most a quarter and 4 KiB larger (take_best_fit)."""
    i = sc.ROW_COUNTS.index(257)
    assert sc.ROW_COUNTS[i - 1] == 300 and 0 in sc.ROW_COUNTS and 5000 in sc.ROW_COUNTS
    assert 257 * 72 < 300 * 72 <= 257 * 72 + 257 * 72 // 4 + 4096


def test_abi_allocates_its_output_buffers_in_one_place():
    """np.zeros / np.empty (and their _like forms, np.full, np.ones) appear in abi.py inside `_out`, and in `_np`'s return of an empty array,
    nowhere else."""
    tree = ast.parse(open(ABI, encoding="utf-8").read(), ABI)
    allocators = {"zeros", "empty", "zeros_like", "empty_like", "full", "full_like", "ones", "ones_like"}
    found = []
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            continue
        for node in ast.walk(fn):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in allocators
                    and isinstance(node.func.value, ast.Name) and node.func.value.id in ("np", "numpy")):
                found.append((fn.name, node.func.attr))
    assert sorted(found) == [("_np", "zeros"), ("_out", "zeros")], found
    # ... and nothing at module level either
    top = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in allocators]
    assert len(top) == 2, len(top)
    out = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_out")
    assert [a.arg for a in out.args.args] == ["shape", "dtype"]
