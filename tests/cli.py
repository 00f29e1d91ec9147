"""Shared by the tests that run the hanamaru-hip program: the one way to start it.  Not a test module."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hanamaru-renderer_amd", "hanamaru-hip")
ASSETS = os.path.join(ROOT, "assets")


def run_cli(args, cwd, timeout=60, missing="fail"):
    """hanamaru-hip with `args` in the directory `cwd` (made if need be); stderr goes into stdout.  missing: what a test makes of a program
    that is not built, "fail" or "skip" (__graft_entry__.build() makes it with libhanamaru_hip.so)."""
    if not os.path.exists(CLI):
        if missing == "skip":
            pytest.skip("CLI not built (needs libhanamaru_hip.so: __graft_entry__.build())")
        pytest.fail("the CLI is not built (__graft_entry__.build() makes it with libhanamaru_hip.so)")
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([CLI] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
