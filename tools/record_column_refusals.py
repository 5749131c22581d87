"""Record what the column-taking entry points answer to bad calls (tests/column_refusal_cases.py) into
tests/golden/column_refusals.json.  The fixture is the contract for refusal order: record it with the library of the commit
whose behaviour is to be kept (TYPLONK_LIB_PATH names another build), on a GPU machine:
    python tools/record_column_refusals.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import typlonk_amd
    from column_refusal_cases import run_cases

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "column_refusals.json")
    ctx = typlonk_amd.Context(0)
    try:
        cases = run_cases(ctx)
    finally:
        ctx.close()
    with open(out, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {out}")


if __name__ == "__main__":
    main()
