"""Records tests/golden/isect/digests.json: the sha256 digests tests/test_isect_host.py holds the host builds of csrc/hr_math.h,
hr_train.h and hr_plan.h to.  Run it on the commit whose bits are the reference -- the one BEFORE a change to the intersection geometry
or the tap index -- and commit the file with the change:

    python tools/make_isect_golden.py

TEST INFRASTRUCTURE ONLY."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import test_isect_host as T  # noqa: E402

if __name__ == '__main__':
    out = {'isect': {T.case_id(*c): T.isect_record(*c) for c in T.CASES}, 'taps': {str(n): T.tap_record(n) for n in T.TAP_SIZES}}
    os.makedirs(os.path.dirname(T.DIGESTS), exist_ok=True)
    with open(T.DIGESTS, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for k, v in out['isect'].items():
        print(k, {a: b for a, b in v.items() if a not in ('dist', 'd_head')})
