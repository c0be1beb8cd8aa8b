"""GPU tests of the acquisition series (gj_acq_series_dev); see test_acq_gpu.py in this package."""
