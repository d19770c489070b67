"""Golden fixture of tests/test_host_trace_cpu.py: the library calls of every configuration of that test as the type-checking
stub of the C ABI records them (names table + per configuration one (name index, argument digest) pair per call).  No GPU, no
reference: the fixture pins what the host layer of the commit it is written at hands to the library.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_host_trace.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)

import test_host_trace_cpu as T  # noqa: E402


def main():
    traces = {}
    for name in T.CONFIGS:
        with T.recording_stub() as lib:
            traces[name] = T.record(name, lib)
        print(f'{name}: {len(traces[name])} calls')
    with open(T.GOLD, 'w') as f:
        json.dump(T.encode(traces), f, separators=(',', ':'))
        f.write('\n')
    print('wrote', T.GOLD, os.path.getsize(T.GOLD), 'bytes')


if __name__ == '__main__':
    main()
