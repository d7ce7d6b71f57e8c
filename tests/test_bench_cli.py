"""bench.py's command line (no GPU: --help ends before anything touches the device): the options a driver relies on are there, --full
(what a plain run leaves out) among them."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_the_contract_and_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    usage = re.sub(r"\s+", " ", r.stdout)
    for opt in ("--gpus GPUS", "--steps STEPS", "--warmup WARMUP", "--dump-outputs DIR", "[--full]"):
        assert opt in usage, opt

