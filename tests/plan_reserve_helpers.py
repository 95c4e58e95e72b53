"""Shared by tests/test_plan_reserve_host.py and tests/test_gpu_plan_reserve.py: the literal tasks of the reservation and retry
tests."""
import numpy as np

# Three 10x10 / 4 tasks that fail under all 24 planning orders of the default rule: a droplet planned earlier steps into the 3x3
# box of a start at Chebyshev distance 2, and the droplet there has no legal action at t = 0.  With one reserved level they route
# in attempt 0, in CORNERED_STEPS steps.
CORNERED_STARTS = np.array([[[8, 3], [7, 1], [6, 8], [9, 7]], [[2, 2], [9, 0], [1, 0], [5, 2]], [[9, 0], [6, 3], [5, 5], [2, 7]]])
CORNERED_GOALS = np.array([[[5, 1], [3, 6], [9, 0], [0, 7]], [[3, 0], [7, 0], [7, 8], [9, 8]], [[3, 5], [8, 9], [0, 0], [5, 0]]])
CORNERED_STEPS = [12, 14, 11]

# A 20x20 / 10 task (of oracle_tasks(20, 20, 10, seed=3)) that no rotation routes at reserve 0 and the second retry does.
RETRY_STARTS = np.array([[[0, 1], [11, 17], [9, 8], [13, 7], [7, 2], [10, 6], [10, 0], [16, 12], [10, 2], [6, 0]]])
RETRY_GOALS = np.array([[[5, 10], [8, 6], [4, 3], [19, 5], [1, 7], [12, 5], [12, 9], [7, 12], [1, 5], [6, 15]]])
