"""bench.py --dump-outputs: what the timed path computed is written as .npy files of at most 64 MB (a larger image as a
fixed, seeded sample of its pixels), identical from run to run for the same image.  The GPU side - the dump of a real run
is its last frame - is tests/test_parity_gpu.py::test_bench_frames_in_flight."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_canvas_is_written_whole(tmp_path):
    bench = _bench()
    image = np.random.default_rng(3).random((1080, 1920, 3))
    assert image.nbytes <= bench.DUMP_LIMIT_BYTES
    assert bench.dump_outputs(str(tmp_path), "canvas", image) == ["canvas.npy"]
    got = np.load(tmp_path / "canvas.npy")
    assert got.dtype == np.float64 and np.array_equal(got, image)


def test_large_image_is_a_seeded_sample_within_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    image = np.random.default_rng(4).random((600, 800, 4)).astype(np.float32)
    runs = []
    for k in range(2):
        out = tmp_path / str(k)
        files = bench.dump_outputs(str(out), "framebuffer_rgba8", image)
        assert files == ["framebuffer_rgba8_sample.npy", "framebuffer_rgba8_sample_pixels.npy"]
        assert sum(os.path.getsize(out / f) for f in files) <= bench.DUMP_LIMIT_BYTES
        runs.append([np.load(out / f) for f in files])
    (sample, pixels), (sample2, pixels2) = runs
    assert sample.dtype == np.float32 and pixels.dtype == np.float64
    assert np.array_equal(sample, sample2) and np.array_equal(pixels, pixels2)
    idx = pixels.astype(np.int64)
    assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < 600 * 800
    assert np.array_equal(sample, image.reshape(-1, 4)[idx])
