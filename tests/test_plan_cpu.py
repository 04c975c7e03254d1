"""The dispatch decisions of csrc/dispatch_plan.h (which k_accel instance, the heavy-tile
split, the lane_k slots, compaction, the samples paths, a dispatch's pixels) against their
stated results, on the CPU (tests/native/plan_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check():
    """All 22 k_accel instances by case and cost, the ladder's priority (MT over per-tile
    records over compaction over latency mode, SS over all), every argument combination one
    of the 22; heavy_split on the frames the measurements name and with each gate closed;
    dispatch_pixels on contiguous, striped and empty dispatches; samples_plan's six flags."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "build/plan_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "build", "plan_check")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_check ok" in r.stdout and " 0 failed" in r.stdout
