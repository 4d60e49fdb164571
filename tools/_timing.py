"""What the timing tools (time_fpfh_ransac.py, time_knn3.py, time_icp_registration.py) share: host clocks around calls that end in a
device synchronise, medians, the device's description, and the driver that runs every step as a child process under ``timeout``."""
import json
import subprocess
import sys
import time


def timed(fn):
    """(milliseconds, result) of one call, a device synchronise before and after"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def median(v):
    return sorted(v)[len(v) // 2]


def med_of(fn, reps=10, warm=3):
    """(median ms, minimum ms, last result) of ``reps`` calls after ``warm`` untimed ones"""
    ts, r = [], None
    for i in range(warm + reps):
        ms, r = timed(fn)
        if i >= warm:
            ts.append(ms)
    return median(ts), min(ts), r


def device_description():
    import torch
    return f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), ROCm {torch.version.hip}, torch {torch.__version__}"


def write_step(path, result, show=0):
    """the child's end: its result and the device it ran on, for run_steps() to read (the first ``show`` characters also printed)"""
    path.write_text(json.dumps(dict(result=result, box=device_description()), indent=1))
    if show:
        print(json.dumps(result)[:show], flush=True)


def run_steps(script, out, steps, extra=()):
    """``script --step [name] --json FILE`` for every (name, limit in seconds) of ``steps``, each a child process of its own under
    ``timeout -k 10 limit``; a non-zero status ends the run.  (status, {name: result}, device description).  An empty name stands for a
    tool whose ``--step`` takes no value; ``extra``: further arguments every child receives."""
    res, box = {}, ""
    for name, limit in steps:
        js = out.with_suffix(f".{name or 'step'}.json")
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(script), "--step", *([name] if name else []),
                             "--json", str(js), *extra]).returncode
        if rc != 0:
            print(f"step {name or 'timing'} ended with status {rc}: stopping", flush=True)
            return rc, res, box
        d = json.loads(js.read_text())
        res[name], box = d["result"], d["box"]
        js.unlink()
    return 0, res, box


def write_report(out, text, data):
    """the rendered table to ``out``, the figures next to it as .json, and the table on the terminal"""
    out.write_text(text)
    out.with_suffix(".json").write_text(json.dumps(data, indent=1))
    print(text)
