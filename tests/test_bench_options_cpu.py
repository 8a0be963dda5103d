"""bench.py's options on CPU: the host-fed steps belong to --full, and asking for them in a plain run is a message before anything
has touched a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_fed_steps_need_full():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for feed in ("host", "both"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--feed", feed], capture_output=True, timeout=120, env=env)
        assert r.returncode == 2 and b"part of --full" in r.stderr, r.stderr.decode()[-1000:]
        assert not r.stdout.strip()
