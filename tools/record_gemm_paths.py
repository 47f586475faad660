"""Record which GEMM kernel every launch of tests/_gemmpaths.py LAUNCHES reaches on this checkout and this device, as
``ops.gemm_last_path`` / ``ops.gemm_last_tail`` report it: the table tests/test_gpu_gemm_plan.py compares against
(tests/golden/gemm_paths_parent.json was recorded with this tool on the commit before the GEMM planner).  One child process
per switch setting, so that a library that latches a switch at its first call records every setting correctly.

    python tools/record_gemm_paths.py OUT.json
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _gemmpaths as P  # noqa: E402


def child(env_key):
    import torch
    import spatial_clip_amd  # noqa: F401
    from spatial_clip_amd import ops
    from tests.test_gpu_gemm_plan import run_launch
    out = {}
    for case in P.LAUNCHES:
        if json.dumps(case[7], sort_keys=True) == env_key:
            out[P.launch_key(case)] = run_launch(ops, case)
    torch.cuda.synchronize()
    print("RECORD " + json.dumps({"slots": torch.cuda.get_device_properties(0).multi_processor_count, "launches": out}))


def main(dst):
    table = {"slots": None, "launches": {}}
    envs = []
    for case in P.LAUNCHES:
        k = json.dumps(case[7], sort_keys=True)
        if k not in envs:
            envs.append(k)
    for k in envs:
        env = {n: v for n, v in os.environ.items() if n not in P.SWITCHES}
        env.update(json.loads(k))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", k], env=env, capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            sys.exit("child %s failed (%d):\n%s\n%s" % (k, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORD ")][-1][7:])
        table["slots"] = rec["slots"]
        table["launches"].update(rec["launches"])
    with open(dst, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d launches under %d settings -> %s" % (len(table["launches"]), len(envs), dst))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1])
