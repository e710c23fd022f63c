"""CPU: everything an MSM decides before its first launch (csrc/msm_plan.h: window layout, option decoding, tables_plan / wide_plan,
bucket_plan, the shape of the two-level reduction), compiled for the HOST with g++ (the header is plain C++): the layout identities
for 10 ... 32 windows, the plans on record as literal values, and every row of tests/native/msm_plan_table.txt -- the planners' full
results over pairs x field x forced option value, recorded before the planners moved into the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_msm_plan_host_selftest(tmp_path):
    exe = str(tmp_path / "msm_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(NATIVE, "msm_plan_selftest.cpp")])
    table = os.path.join(NATIVE, "msm_plan_table.txt")
    with open(table) as f:
        recorded = f.read().splitlines()
    # 11 pair counts x 2 fields x 11 option values, then 4 pieces x 9 option values of the wide planner; "no plan" rows included
    assert len(recorded) == 11 * 2 * 11 + 4 * 9
    assert sum(1 for r in recorded if r.split(" : ")[1].startswith("0 ")) > 0
    out = subprocess.run([exe, table], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "layout identities: 0 failures" in out.stdout, out.stdout
    assert "anchors: 0 failures" in out.stdout, out.stdout
    assert "recorded table: 0 failures of %d rows" % len(recorded) in out.stdout, out.stdout
    # the print mode writes the same table
    printed = subprocess.run([exe, "--print"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert printed == recorded
