"""CPU: bench.py's command line -- a plain run leaves the extra legs to --full, and --dump-outputs writes the proof as float32
arrays (tests/test_gpu_parity.py::test_bench_plain_run_is_lean_and_dumps_the_last_proof runs both on the GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(monkeypatch, argv):
    monkeypatch.syspath_prepend(ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    import bench
    return bench


def test_full_is_off_by_default_and_dump_outputs_is_optional(monkeypatch):
    bench = _bench(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "1", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_the_proof_bytes_and_bits(monkeypatch, tmp_path):
    bench = _bench(monkeypatch, [])
    for curve, size in (("bls12_381", 176), ("bn254", 128)):
        proof = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8).tobytes()
        out = tmp_path / curve
        bench.dump_outputs(str(out), curve, proof)
        b, bits = np.load(out / "proof.npy"), np.load(out / "proof_bits.npy")
        assert b.dtype == np.float32 and bits.dtype == np.float32
        assert b.astype(np.uint8).tobytes() == proof
        assert bits.shape == (8 * size,) and set(np.unique(bits)) <= {0.0, 1.0}
        assert np.packbits(bits.astype(np.uint8), bitorder="little").tobytes() == proof
