"""Write what the Franka solver wrappers and collision checks hand to the C library, over the fixed grid of
tests/solver_call_grid.py, as JSON: to show that a change of the Python host layer changes no call.  Runs without a GPU (the
library call is recorded, not made).

    python tools/solver_calls.py OUT.json

Run it from two trees (copy this file and tests/solver_call_grid.py into the older one) and compare the two files byte for
byte.  Per call: the entry name, every integer and float as passed, option structs by field, and each pointer as None,
``input:<argument name>+<byte offset>`` or ``other``.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests")]


def main():
    import solver_call_grid as grid

    rows = []
    for case, thunk, inputs in grid.cases():
        with grid.recording() as calls:
            thunk()
        rows.append({"case": case, "calls": [grid.describe(n, a, inputs) for n, a in calls]})
    calls, inputs, _ = grid.slabbed_plan_cloud()
    rows.append({"case": f"franka_plan_cloud B{grid.SLAB_B} under {grid.SLAB_ROWS} problems' scratch",
                 "calls": [grid.describe(n, a, inputs) for n, a in calls]})
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
    print(f"{len(rows)} cases, {sum(len(r['calls']) for r in rows)} calls -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
