"""Host side of the data set path (the reference's `datapipe/` package): directory trees, splits and index streams. The
per-sample transforms of the reference's loader workers run on the device (device_pipeline.py, resident_pool.py)."""
