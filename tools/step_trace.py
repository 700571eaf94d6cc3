"""Record what Engine.step sends to the device in every mode (tests/step_trace_ref.py: calls with arguments, sync waits,
read-backs) into tests/golden/step_trace.json.gz, the fixture of tests/test_step_trace_gpu.py.  Record it on the commit whose
step is the yardstick (the parent of a refactor), never on the code under test; the tool touches only attributes every version
of the step keeps.      GPU box: python tools/step_trace.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tiny-newsrec_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import step_trace_ref as S      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_trace.json.gz"))
a = ap.parse_args()
traces = {}
for name in S.scenarios():
    traces[name] = S.run(name)
    print("%-40s %3d entries, %3d calls" % (name, len(traces[name]), sum(e[0] == "call" for e in traces[name])))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
S.save(a.out, traces)
print("%d scenarios, %d bytes of JSON -> %s (%d bytes)" % (len(traces), len(S.dumps(traces)), a.out, os.path.getsize(a.out)))
