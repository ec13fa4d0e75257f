"""Mirror of deepim/core: the test loop (tester.py) and the training loop (module.py, metric.py, callback.py)."""
