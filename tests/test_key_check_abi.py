"""CPU: the boundary of PM_KEY_CHECK_RELATIONS -- one flag value in pm_pk_load_bytes' `validate`, no entry point, option, status value
or getenv of its own -- and the host mirror of the check (polymath_amd/host/key_check.hpp): the g++ self-test (keys made by a literal
restatement of the generator at n = 8 and 16 on both curves, every tamper refused by name, the ChaCha12 text against the published
vector and StdRng), once more as a stand-alone program under AddressSanitizer and UBSan, and the mirror over every key of
tests/golden/pk_wire.json: valid inputs pass on the reference's own bytes."""
import inspect
import os
import re
import subprocess

import pytest

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
RUST_SYS = os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")
RUST_WRAPPER = os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")
NATIVE = os.path.join(ROOT, "tests", "native")


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_flag_is_the_same_constant_everywhere():
    from polymath_amd import api
    header = open(HEADER).read()
    m = re.search(r"typedef enum pm_key_check \{(.*?)\} pm_key_check;", _code(header), flags=re.S)
    assert m and dict(re.findall(r"(PM_KEY_CHECK_[A-Z]+)\s*=\s*(\d+)", m.group(1))) == {"PM_KEY_CHECK_NONE": "0", "PM_KEY_CHECK_RELATIONS": "512"}
    assert header.index("} pm_wire_form;") < header.index("typedef enum pm_key_check") < header.index("int pm_g1_decode(")
    assert (api.PM_KEY_CHECK_NONE, api.PM_KEY_CHECK_RELATIONS) == (0, 512)
    assert api.PM_KEY_CHECK_RELATIONS & (api.PM_WIRE_UNCOMPRESSED | 1) == 0
    sys_rs = open(RUST_SYS).read()
    assert dict(re.findall(r"pub const (PM_KEY_CHECK_[A-Z]+): i32 = (\d+);", sys_rs)) == {"PM_KEY_CHECK_NONE": "0", "PM_KEY_CHECK_RELATIONS": "512"}


def test_wrappers_carry_the_flag():
    from polymath_amd import api
    from polymath_amd import polymath as PM
    for fn in (api.ProvingKey.load_bytes, PM.Polymath.pk_load_bytes):
        p = inspect.signature(fn).parameters
        assert "relations" in p and p["relations"].default is False and list(p)[-1] == "relations"
    wrapper = open(RUST_WRAPPER).read()
    body = wrapper[wrapper.index("pub fn load_bytes_checked<E: Pairing>"):]
    body = body[:body.index("\n    }") + 6]
    assert "sys::PM_KEY_CHECK_RELATIONS" in body and "1 |" in body
    assert len(re.findall(r"sys::pm_pk_load_bytes\s*\(", wrapper)) == 1          # one call site, three public ways in


def test_header_contract_phrases():
    header = open(HEADER).read()
    doc = header[header.index("PM_KEY_CHECK_RELATIONS is a FLAG"):header.index("typedef enum pm_key_check")]
    doc = " ".join(doc.replace("\n *", " ").split())
    for phrase in ("OR-ed into the `validate` argument of pm_pk_load_bytes only", "there is no entry point of its own",
                   "BEFORE the window tables are built", "validation is on iff (validate & ~256) != 0", "the flag implies point validation",
                   "It combines with PM_WIRE_UNCOMPRESSED", "pm_g1_decode ignores it", "With shard_count > 1",
                   "PM_ERR_INVALID_ARG, no handle, nothing stays allocated", "FIRST failing relation", "getrandom(2)", "PM_ERR_STATE",
                   "ChaCha12", "Out of scope: sharded keys", "already resident from pm_pk_load", "a caller-supplied seed",
                   "a vk supplied separately from the key",
                   "x_powers_g1: the first entry is not vk.one_g1", "consecutive entries are not in ratio x",
                   "is not anchored to vk.one_g1 and vk.z_g2", "uj_wj_lcs_by_y_alpha_g1: does not match the SAP matrices"):
        assert phrase in doc, phrase
    # the sentence the uncompressed form wrote stays as it was
    assert "validation is on iff (validate & ~256) != 0, so 0 and 1 mean what they always meant" in " ".join(header.replace("\n *", " ").split())
    # the texts are the mirror's
    mirror = open(os.path.join(ROOT, "polymath_amd", "host", "key_check.hpp")).read()
    for text in (": the first entry is not vk.one_g1", ": consecutive entries are not in ratio x", ": is not anchored to vk.one_g1 and vk.z_g2",
                 ": does not match the SAP matrices"):
        assert mirror.count('"' + text + '"') == 1, text
    for doc_file, anchor in (("README.md", "PM_KEY_CHECK_RELATIONS"), ("DESIGN.md", "PM_KEY_CHECK_RELATIONS")):
        assert anchor in open(os.path.join(ROOT, doc_file)).read(), doc_file


def test_pinned_counts_did_not_move():
    from polymath_amd import api
    code = _code(open(HEADER).read())
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70 == len(api.EXPORTS)
    assert len(api.OPTIONS) == 9 and len(re.findall(r"\bPM_OPT_[A-Z_]+\s*=\s*\d+", code)) == 9
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    sys_rs = open(RUST_SYS).read()
    assert len(set(re.findall(r"pub fn (pm_[a-z0-9_]+)", sys_rs[sys_rs.index('extern "C" {'):]))) == 70
    # the check reads no environment variable of its own, and draws from the operating system in one place
    csrc = os.path.join(ROOT, "polymath_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "key_check.hip")).read()
    assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "host", "key_check.hpp")).read()
    assert sum(open(os.path.join(csrc, f)).read().count("getrandom(") for f in os.listdir(csrc)) == 1
    from polymath_amd import build as pb
    assert "key_check.hip" in pb.SOURCES


def test_chacha_rounds_are_stated_once():
    host = os.path.join(ROOT, "polymath_amd", "host")
    csrc = os.path.join(ROOT, "polymath_amd", "csrc")
    rotations = 0
    for d in (host, csrc):
        for f in os.listdir(d):
            rotations += len(re.findall(r"chacha_rotl\(x\[d\] \^ x\[a\], 16\)", open(os.path.join(d, f)).read()))
    assert rotations == 1
    assert "chacha12_weight" in open(os.path.join(csrc, "key_check.hip")).read()


@pytest.mark.parametrize("flags, args", [(["-O2"], []), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["--quick"])],
                         ids=["plain", "sanitized"])
def test_key_check_host_selftest(tmp_path, flags, args):
    exe = str(tmp_path / "key_check_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-pthread"] + flags + ["-o", exe, os.path.join(NATIVE, "key_check_selftest.cpp")])
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    shapes = ["bls12_381 n=8"] if args else ["bls12_381 n=8", "bls12_381 n=16", "bn254 n=8", "bn254 n=16"]
    for shape in shapes:                                     # 1 valid + 1 swap + 6 x 3 + 4 lcs entries + 3 vk + 1 matrices
        assert shape + ": 28 keys checked" in lines, out.stdout
    # per shape 28 verdicts and the unused column's infinity; 3 ChaCha checks
    assert "key check selftest: 0 failures of %d" % (3 + 29 * len(shapes)) in lines, out.stdout


def test_mirror_accepts_every_fixture_key(tmp_path):
    """The condition that valid inputs pass, on the reference's own bytes, before any GPU run."""
    exe = str(tmp_path / "key_check_runner")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(NATIVE, "key_check_runner.cpp")])
    keys = load_golden("pk_wire.json")["keys"]
    assert len(keys) >= 5
    # one process a key (hex through stdin), side by side: the host pairing is slow
    procs = [subprocess.Popen([exe, "bls12_381", "compressed"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for _ in keys]
    for p, k in zip(procs, keys):
        p.stdin.write(k["pk_bytes"] + "\n")
        p.stdin.close()
    for p, k in zip(procs, keys):
        out = p.stdout.read()
        assert p.wait() == 0 and out.splitlines() == ["ok"], (k["name"], out)
    # argv, and a key that is no proving key: the first x power doubled is caught by name (bytes 392 + header .. are the matrices;
    # the runner is given a truncated key too)
    hexkey = keys[0]["pk_bytes"]
    out = subprocess.run([exe, "bls12_381", "compressed", hexkey[:-2]], capture_output=True, text=True)
    assert out.returncode == 1 and out.stdout.startswith("malformed: "), out.stdout
    out = subprocess.run([exe, "bls12_381", "uncompressed", hexkey], capture_output=True, text=True)
    assert out.returncode == 1 and out.stdout.startswith("malformed: "), out.stdout
