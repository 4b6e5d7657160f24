"""bench.py's command line: a plain run stops at the headline line; the oracle checks, CPU baselines and secondary
workloads run only with --full."""
import bench


def test_full_is_off_by_default():
    assert bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "3"]).full is False
    assert bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"]).full is True
