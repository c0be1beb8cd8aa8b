"""GPU tests of the acquisition search at the edges of its peak test (see test_acq_gpu.py)."""
