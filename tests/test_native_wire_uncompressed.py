"""CPU: the uncompressed wire form of the host mirror (polymath_amd/host/wire.hpp: ser_g1_uncompressed, deser_g1_uncompressed, the G2
pair, read_vk_c / ser_vk_c / WireKey with a form), compiled with g++ from tests/native/wire_uncompressed_selftest.cpp.  The four
literal records (both generators, both infinities) both ways; deser_u(ser_u(kG)) == deser_c(ser_c(kG)) for k = 1 .. 64 and for
(x, -y), on both curves; every refusal with its text -- the compressed bit, the sort bit on a finite point and on infinity, stray
bits in either half and in the flag byte of infinity, x = p, y = p, p + 1, the all-ones coordinate, BN254's two flag bits, (x, y + 1)
off the curve -- with validation on AND off; a BLS12-381 curve point outside G1, refused validated and accepted unvalidated; BN254's
"y > -y" bit set and clear on the same point, both accepted; G2 in both forms, off the twist, infinity; the vk at 392 / 728 and
280 / 504 bytes, transcoded both ways, and refused in the other form; every key of tests/golden/pk_wire.json parsed, written
uncompressed (length = compressed + 48 per point + 336), parsed again, written compressed: the original bytes -- and refused in the
wrong form, truncated, or with a trailing byte.  Once more as a stand-alone program under AddressSanitizer and UBSan (one key)."""
import os
import subprocess

import pytest

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "wire_uncompressed_selftest.cpp")


@pytest.mark.parametrize("flags, keys", [(["-O2"], None), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ("dummy",))],
                         ids=["plain", "sanitized"])
def test_wire_uncompressed_host_selftest(tmp_path, flags, keys):
    files = []
    for key in load_golden("pk_wire.json")["keys"]:
        if keys is None or key["name"] in keys:
            path = tmp_path / ("pk_%s.hex" % key["name"])
            path.write_text(key["pk_bytes"])
            files.append(str(path))
    assert files
    exe = str(tmp_path / "wire_uncompressed_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # literals 4; k G 64 x 2 (x 2 on BN254: the sign bit); refusals 2 x 13 / 2 x 11; subgroup 3 / sign bit 1; truncated 1;
    # G2 3 x 3 / 3 x 2, infinity 2; vk 6
    lines = out.stdout.splitlines()
    assert "bls12_381: 0 failures of 179" in lines and "bn254: 0 failures of 298" in lines, out.stdout
    assert out.stdout.count("wire ok") == len(files) and "wire uncompressed selftest: 0 failures" in lines, out.stdout
