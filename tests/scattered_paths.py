"""How the tests of modelnum 4 choose between its two cooperative stencil paths (tests/test_gpu_scattered_paths.py,
test_gpu_scattered_tier.py).  Not a test module."""
import os


def _own_list(fn):
    """Run fn() with the staging buffer switched off (own-list path for every stencil)."""
    os.environ["SRT_SCATTERED_STAGING"] = "0"
    try:
        return fn()
    finally:
        del os.environ["SRT_SCATTERED_STAGING"]
