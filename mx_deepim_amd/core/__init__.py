"""Mirror of deepim/core: the test loop (tester.py)."""
