"""Electrode-degradation sweep with the loop of the reference's evaDegre.py (:8-56), vectorised.

The reference ages 5 chips one after another: per chip `evaluate_epoch` epochs, per epoch it
snapshots `routing_manager.m_health` and plays `evaluate_task` greedy episodes on the SAME chip, so
usage accumulates and `updateHealth` (dmfb.py:465-471) degrades electrodes between episodes.  Here
every chip of a `VecDMFB(b_degrade=True, per_degrade=1.0)` batch ages in parallel; the outputs have
the reference's layout with the chip axis first:
    rewards/steps/success: (chips, epochs)      health: (chips, epochs, W, L)
and are saved under the reference's file names (rewards.npy, steps.npy, success.npy, health.npy in
DegreData/{W}by{W}-{n}d{b}b/).

`--router follow [--min_health X]` ages the chips under the closed-loop planner (marl_dmfb_amd.plan.Follower) instead of a policy:
no checkpoint is loaded, the loop and the four files are the same, under DegreData_follow/, so that tools/compare_degre.py reads
them beside the policy's.  `--reserve R` / `--retries Q` give the follower the two opt-in parameters of the planning rule."""
import os

import numpy as np
import torch

from .common.rollout import Evaluator


class Degre_evaluator(Evaluator):
    def __init__(self, env, agents, args):
        super().__init__(env, agents, args.episode_limit)
        self.evaluate_epoch = int(args.evaluate_epoch)
        self.evaluate_task = int(args.evaluate_task)
        self.shield = bool(getattr(args, 'shield', False))
        self.meda_shield = bool(getattr(args, 'meda_shield', False))

    def evaluate_process(self):
        E = self.n_envs
        W, L = self.env.width, self.env.length
        rewards = torch.zeros((E, self.evaluate_epoch), dtype=torch.float64, device=self.device)
        steps = torch.zeros_like(rewards)
        success = torch.zeros_like(rewards)
        health = torch.zeros((E, self.evaluate_epoch, W, L), dtype=torch.float64, device=self.device)
        for epoch in range(self.evaluate_epoch):
            health[:, epoch] = self.env.get_map('health')            # evaDegre.py:21
            for _ in range(self.evaluate_task):                       # Evaluator.evaluate (rollout.py:69-85)
                r, s, _, ok = self._generate_episode()
                rewards[:, epoch] += r
                steps[:, epoch] += s.double()
                success[:, epoch] += ok.double()
            rewards[:, epoch] /= self.evaluate_task
            steps[:, epoch] /= self.evaluate_task
            success[:, epoch] /= self.evaluate_task
        return rewards.cpu().numpy(), steps.cpu().numpy(), success.cpu().numpy(), health.cpu().numpy()


class Degre_follower:
    """The sweep of Degre_evaluator with a plan.Follower in place of the policy: reset(new=False) between the episodes, so the
    chips age, and record=True, so usage accumulates."""

    def __init__(self, env, args):
        from .plan import Follower
        self.env, self.follower = env, Follower(env, min_health=float(args.min_health), reserve=getattr(args, 'reserve', 0),
                                                retries=getattr(args, 'retries', 0))
        self.evaluate_epoch, self.evaluate_task = int(args.evaluate_epoch), int(args.evaluate_task)

    def evaluate_process(self):
        env = self.env
        E, W, L, dev = env.n_envs, env.width, env.length, env.device
        rewards = torch.zeros((E, self.evaluate_epoch), dtype=torch.float64, device=dev)
        steps = torch.zeros_like(rewards)
        success = torch.zeros_like(rewards)
        health = torch.zeros((E, self.evaluate_epoch, W, L), dtype=torch.float64, device=dev)
        for epoch in range(self.evaluate_epoch):
            health[:, epoch] = env.get_map('health')
            for _ in range(self.evaluate_task):
                env.reset(new=False)
                res = self.follower.play(record=True)
                rewards[:, epoch] += res.reward
                # a failed episode counts the whole limit, as Evaluator._play counts it
                steps[:, epoch] += torch.where(res.success, res.steps, torch.full_like(res.steps, env.max_step)).double()
                success[:, epoch] += res.success.double()
        n = self.evaluate_task
        return (rewards / n).cpu().numpy(), (steps / n).cpu().numpy(), (success / n).cpu().numpy(), health.cpu().numpy()


def save_results(args, rewards, steps, success, health, root='DegreData'):
    path = os.path.join(root, '{}by{}-{}d{}b'.format(args.width, args.width, args.drop_num, args.block_num))
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'rewards.npy'), rewards)
    np.save(os.path.join(path, 'steps.npy'), steps)
    np.save(os.path.join(path, 'success.npy'), success)
    np.save(os.path.join(path, 'health.npy'), health)
    return path


def main(argv=None):
    from .agent.agent import Agents
    from .common.arguments import get_evaluate_args
    from .env.dmfb import VecDMFB
    args = get_evaluate_args(argv)
    n_chips = getattr(args, 'n_envs', 5)
    env = VecDMFB(args.width, args.length, args.drop_num, args.block_num, fov=args.fov, stall=args.stall,
                  b_degrade=True, per_degrade=1.0, n_envs=n_chips, seed=1)
    args.__dict__.update(env.get_env_info())
    if args.alg == 'qmix':
        args.state_shape = env.state_shape   # the mixer is loaded with the checkpoint; greedy play uses the agent network only
    args.device = str(env.device)
    if getattr(args, 'router', None) == 'follow':
        print('saved to', save_results(args, *Degre_follower(env, args).evaluate_process(), root='DegreData_follow'))
        return
    agents = Agents(args)
    ev = Degre_evaluator(env, agents, args)
    out = ev.evaluate_process()
    print('saved to', save_results(args, *out))


if __name__ == '__main__':
    main()
