"""Shared by tests/test_meda_follow_wide_host.py and tests/test_gpu_meda_follow_wide.py: the cases of the wide MEDA closed-loop
router (chips above 64 rows or columns; tasks as the CPU oracle draws them, a seeded health map and seeded move draws) and their
follow_reference_meda results, computed once per process."""
import functools

from follow_helpers import FIELDS, build_case, build_reference, equal  # noqa: F401  (all as for the narrow follower)
from meda_plan_helpers import oracle_tasks

# name -> chip, tasks, health range, min_health, as meda_follow_helpers.CASES.  `seam`: the axis (0 x, 1 y) along which recorded
# centres must pass 63, the last column of a row's first word or the last row a lane holds as its first.
# 20x72 / 72x20 cross one seam each on a cheap chip, 128x20 / 20x128 reach the far clamp (centre 125), 128x128 and 80x80 (the
# reference's default chip for ten droplets) cross both, 65x65 is the first size past the narrow follower, the two min_health
# cases force parking (see meda_follow_helpers.CASES for `worn`), and 20x72_3_many has more chips than a launch has workgroups
# (512): walks of 2 and 3 chips.  128x128 / 16 is left out: its reference takes minutes for one chip.
CASES = {
    '20x72_3': dict(width=20, length=72, n_agents=3, seed=51, B=16, low=0.6, seam=(0,)),
    '72x20_3': dict(width=72, length=20, n_agents=3, seed=52, B=16, low=0.6, seam=(1,)),
    '128x20_3': dict(width=128, length=20, n_agents=3, seed=57, B=8, low=0.6, seam=(1,)),
    '20x128_3': dict(width=20, length=128, n_agents=3, seed=58, B=8, low=0.6, seam=(0,)),
    '128x128_3': dict(width=128, length=128, n_agents=3, seed=55, B=2, low=0.6, seam=(0, 1)),
    '80x80_10': dict(width=80, length=80, n_agents=10, seed=54, B=2, low=0.6, seam=(0, 1)),
    '65x65_9': dict(width=65, length=65, n_agents=9, seed=59, B=4, low=0.6, seam=()),
    '20x100_4_min_health': dict(width=20, length=100, n_agents=4, seed=56, B=16, low=0.2, min_health=0.9, worn=0.02, seam=(0,)),
    '100x20_4_min_health': dict(width=100, length=20, n_agents=4, seed=61, B=16, low=0.2, min_health=0.9, worn=0.02, seam=(1,)),
    '20x72_3_many': dict(width=20, length=72, n_agents=3, seed=60, B=1032, unique=129, low=0.6, seam=(0,)),
}
# the cases run with fewer levels in LDS than fit: plans whose levels live in the workspace
FEW_LEVELS = ('128x20_3', '20x128_3', '80x80_10')


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, starts, goals, health, uniforms) of a case; the arrays are shared: do not write to them."""
    c = CASES[name]
    W, L = c['width'], c['length']
    s, g, _, health, uniforms = build_case(c, lambda m: (*oracle_tasks(W, L, c['n_agents'], c['seed'], B=m), None), W + L)
    return c, s, g, health, uniforms


@functools.lru_cache(maxsize=None)
def reference(name):
    """follow_reference_meda of a case, computed once per process."""
    from marl_dmfb_amd.plan import follow_reference_meda
    c, s, g, health, uniforms = case(name)
    return build_reference(c, s, g, None, health, uniforms, lambda W, L, s, g, blocks, **kw: follow_reference_meda(W, L, s, g, **kw))
