"""CPU: everything a proving key decides before its first allocation (host/key_plan.hpp: key_plan -- domain, base concatenation, MSM
ranges, resident pieces, quotient segments of all ranks -- and table_grants, which merged MSM gets window tables, which the wide mode),
compiled for the HOST with g++ (the header is plain C++): the identities over n = 2^2 ... 2^14 x ranks x m0 x layouts x sub-segment
sizes with the refused arguments, the grants on record as literal values, and every row of tests/native/key_plan_table.txt -- full plans
and grants recorded from api.hip before they moved into the header.  Once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_key_plan_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "key_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(NATIVE, "key_plan_selftest.cpp")])
    table = os.path.join(NATIVE, "key_plan_table.txt")
    with open(table) as f:
        recorded = f.read().splitlines()
    # K rows: 5 circuits x 2 layouts x (1 + 2 + 4 + 8) ranks, 2 circuits x 2 sub-segment sizes x 2 ranks, 6 refusals;
    # G rows: 4 resident sets x (4 free sizes x 4 modes x (3 contexts in flight + bn254 + small pieces) + 2 x 2 x 2 forced x 2 piece sizes)
    assert len(recorded) == (5 * 2 * 15 + 2 * 2 * 2 + 6) + 4 * (4 * 4 * 5 + 2 * 2 * 2 * 2) == 548
    grants = [cell.split()[0] for r in recorded if r.startswith("G ") for cell in r.split(" : ")[1:]]
    assert {"none", "tables", "wide"} == set(grants) and min(grants.count(k) for k in ("none", "tables", "wide")) > 100
    # refused: the 6, and N^2 > n in the grid (PM_SHARD_VECTOR: 4 and 8 ranks at n = 8, 8 ranks at n = 32)
    assert sum(1 for r in recorded if r.startswith("K ") and r.split(" : ")[1] != "0") == 6 + 4 + 8 + 8
    out = subprocess.run([exe, table], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "identities: 0 failures of 544 cases" in out.stdout, out.stdout
    assert "anchors: 0 failures" in out.stdout, out.stdout
    assert "recorded table: 0 failures of %d rows" % len(recorded) in out.stdout, out.stdout
    # the print mode writes the same table
    printed = subprocess.run([exe, "--print"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert printed == recorded
