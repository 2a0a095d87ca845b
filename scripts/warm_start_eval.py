#!/usr/bin/env python3
"""What a DAgger warm start buys: ``voxnav.imitate.warm_start`` on a training room
set, then train/evaluate_grid.py's results table on an evaluate set for the warm-started policy,
the same policy untrained, and the frontier planner that taught it (the row of DESIGN.md 10.3).

The policy is the reference's (``--policy lstm``: RecurrentActorCriticPolicy, LSTM 256, pi / vf
[256, 256, 128]; ``mlp``: ActorCriticPolicy with the same MLP).  beta falls linearly from 1 by
--beta-step per iteration down to --beta-min.  --episodes agents per evaluation, agent i reset with
seed + i, one deterministic episode each, L 10.  --labels set trains on the planner's set of equally
short actions (vn_plan_frontier_dists, vn_bc_loss_set) instead of its lowest-k action.  --labels soft
--label-tau TAU trains on the distance-weighted target of vn_bc_loss_soft; --execute best
(with --labels set or soft) executes the policy's own sample whenever it is among the shortest actions
(vn_dagger_mix_best) and prints own_best_rate per iteration; with either, the warm-started policy gets a
stochastic evaluation row (sampled actions) beside the deterministic one.

--then ppo | kickstart --then-iterations K: after the warm start, K more iterations
on the same collector at beta = 0 with a fresh learner of the reference's PPO hyperparameters --
plain ``ppo.learn``, or ``imitate.kickstart`` with bc_coef = --bc-decay ^ iteration -- and one more
table row for the policy after them.  --action-masks (with --then ppo): the then-phase
collects with invalid-action masking -- a ``RolloutCollector(action_masks=True)`` on the same env (the
DAgger collector has no masks; it starts from a fresh reset), ``PPOLearner(action_masks=True)`` -- and
its table row is evaluated with masks too.  --action-masks with --then kickstart: masked
DAgger and masked kickstart -- the warm start runs on a ``MaskedDaggerCollector`` with
``BCLearner(action_masks=True)``, the then-phase continues on the same collector with
``KickstartLearner(action_masks=True)``, and every evaluation of the policy is masked (the final weights are
evaluated without masks as well).  --target-kl, --clip-range-vf, --lr-schedule linear: the
then-phase's learner stops a train() once a minibatch's approximate KL exceeds 1.5 target_kl, clips the value
update (--then ppo only), and lets the learning rate fall linearly to 0 over the then-phase; the then-phase's
epochs actually run and the seconds spent in train() are printed and reported.  Prints the per-iteration rows, the table and one JSON line.
Needs a GPU."""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "3d-navigation-reinforcement-learning_amd"))
import torch  # noqa: E402

from voxnav.collector import RolloutCollector  # noqa: E402
from voxnav.env import BatchedGridEnv  # noqa: E402
from voxnav.evaluate import RESULTS_HEADER, evaluate_policy, results_table_row  # noqa: E402
from voxnav.imitate import (BCLearner, DaggerCollector, KickstartLearner, MaskedDaggerCollector, kickstart,  # noqa: E402
                            warm_start)
from voxnav.normalize import RewardNormalizer  # noqa: E402
from voxnav.planner import evaluate_planner  # noqa: E402
from voxnav.ppo import PPOLearner, learn  # noqa: E402
from voxnav.policy import ActorCriticPolicy, RecurrentActorCriticPolicy  # noqa: E402
from voxnav.rooms import load_archive_set  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-set", default="P1_training")
    ap.add_argument("--eval-set", default="P1_evaluate")
    ap.add_argument("--policy", choices=["lstm", "mlp"], default="lstm")
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--vf-coef", type=float, default=0.5)
    ap.add_argument("--beta-step", type=float, default=0.05)
    ap.add_argument("--beta-min", type=float, default=0.2)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--labels", choices=["action", "set", "soft"], default="action",
                    help="set: the planner's set of equally short actions as the label (DESIGN.md 10.5); "
                         "soft: the distance-weighted target (DESIGN.md 10.11)")
    ap.add_argument("--label-tau", type=float, default=1.0, help="--labels soft: the target's temperature")
    ap.add_argument("--execute", choices=["expert", "best"], default="expert",
                    help="best: the policy's own sample is executed wherever it is among the shortest actions")
    ap.add_argument("--norm-reward", action="store_true",
                    help="VecNormalize(norm_reward=True) on the rollout's rewards (DESIGN.md 10.6)")
    ap.add_argument("--then", choices=["ppo", "kickstart"], default=None,
                    help="after the warm start: plain PPO, or PPO with the decaying cross-entropy (DESIGN.md 10.7)")
    ap.add_argument("--then-iterations", type=int, default=8)
    ap.add_argument("--bc-decay", type=float, default=0.7, help="kickstart: bc_coef = bc_decay ^ iteration")
    ap.add_argument("--action-masks", action="store_true",
                    help="--then ppo with invalid-action masking, evaluated with masks too (DESIGN.md 10.8); "
                         "--then kickstart: masked DAgger and masked kickstart throughout (DESIGN.md 10.9)")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="the then-phase's learner: stop a train() at approx_kl > 1.5 target_kl (DESIGN.md 10.10)")
    ap.add_argument("--clip-range-vf", type=float, default=None, help="--then ppo: clip the value update")
    ap.add_argument("--lr-schedule", choices=["constant", "linear"], default="constant",
                    help="linear: the then-phase's learning rate falls to 0 with the remaining progress")
    args = ap.parse_args()
    if args.action_masks and args.then is None:
        raise SystemExit("--action-masks goes with --then ppo or --then kickstart")
    if (args.target_kl is not None or args.clip_range_vf is not None or args.lr_schedule != "constant") and \
            args.then is None:
        raise SystemExit("--target-kl, --clip-range-vf and --lr-schedule go with --then ppo or --then kickstart")
    if args.clip_range_vf is not None and args.then == "kickstart":
        raise SystemExit("--clip-range-vf goes with --then ppo (no fused PPO+BC loss clips the value update)")
    masked_imitation = args.action_masks and args.then == "kickstart"
    if not torch.cuda.is_available():
        raise SystemExit("warm_start_eval.py needs a GPU")
    dev = "cuda:0"
    torch.manual_seed(args.seed)
    pol = (RecurrentActorCriticPolicy() if args.policy == "lstm" else ActorCriticPolicy()).to(dev)
    eval_rooms = load_archive_set(args.eval_set)
    kw = dict(n_episodes=args.episodes, local_map_length=args.L, seed=args.seed, device=dev)
    ekw = dict(kw, action_masks=True) if masked_imitation else kw       # the policy's evaluations
    how = ", masked evaluation" if masked_imitation else ""
    rows = {"untrained policy" + how: evaluate_policy(pol, eval_rooms, **ekw)}

    env = BatchedGridEnv(num_agents=args.agents, rooms=load_archive_set(args.train_set), local_map_length=args.L,
                         device=dev)
    rnorm = RewardNormalizer(args.agents, 0.99, device=dev) if args.norm_reward else None
    col = (MaskedDaggerCollector if masked_imitation else DaggerCollector)(env, pol, n_steps=args.n_steps,
                                                                           labels=args.labels, execute=args.execute,
                                                                           reward_norm=rnorm)
    ln = BCLearner(pol, learning_rate=args.lr, n_epochs=args.epochs, batch_size=args.batch, vf_coef=args.vf_coef,
                   seed=args.seed, labels=args.labels, action_masks=masked_imitation, label_tau=args.label_tau)
    t0 = time.time()

    def show(it, done, st):
        keys = ("beta", "expert_share", "own_best_rate", "labelled", "bc_loss", "accuracy", "value_loss", "grad_norm", "ep_finished_rate",
                "ep_bumps_mean", "ep_coverage", "ret_rms_var")
        print(f"iter {it:3d} steps {done:9d} " + " ".join(f"{k}={st[k]:.4g}" for k in keys if k in st), flush=True)

    hist = warm_start(col, ln, total_timesteps=args.iterations * args.agents * args.n_steps,
                      beta=lambda i: max(args.beta_min, 1.0 - args.beta_step * i), callback=show)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    tag = ((" (set labels)" if args.labels == "set" else f" (soft labels, tau {args.label_tau:g})"
            if args.labels == "soft" else "") + (" (best-set execution)" if args.execute == "best" else "") +
           (" (normalised rewards)" if args.norm_reward else ""))
    name = ("masked warm start" if masked_imitation else "warm-started policy") + how + tag
    rows[name] = evaluate_policy(pol, eval_rooms, **ekw)
    if args.labels == "soft" or args.execute == "best":
        rows[name + ", stochastic evaluation"] = evaluate_policy(pol, eval_rooms, deterministic=False, **ekw)
    then_hist, then_s, learn_s = [], 0.0, [0.0]

    def timed_train(learner):
        """learner.train with its wall time (device-synchronised) added to learn_s"""
        train = learner.train

        def run(*a, **k):
            torch.cuda.synchronize()
            t = time.time()
            out = train(*a, **k)
            torch.cuda.synchronize()
            learn_s[0] += time.time() - t
            return out

        learner.train = run
        return learner

    if args.then is not None:
        def show_then(it, done, st):
            keys = ("bc_coef", "loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "bc_loss",
                    "accuracy", "grad_norm", "epochs_run", "n_minibatches", "ep_finished_rate", "ep_bumps_mean", "ep_coverage", "ret_rms_var")
            print(f"{args.then} iter {it:3d} steps {done:9d} " + " ".join(f"{k}={st[k]:.4g}" for k in keys if k in st),
                  flush=True)

        col.set_beta(0.0)
        steps = args.then_iterations * args.agents * args.n_steps
        lr = (lambda p: args.lr * p) if args.lr_schedule == "linear" else args.lr
        hyper = dict(learning_rate=lr, n_epochs=args.epochs, batch_size=args.batch, vf_coef=args.vf_coef,
                     seed=args.seed, target_kl=args.target_kl)
        ppo_hyper = dict(hyper, clip_range_vf=args.clip_range_vf)
        t1 = time.time()
        if args.then == "kickstart":
            kl = timed_train(KickstartLearner(pol, labels=args.labels, action_masks=masked_imitation,
                                              label_tau=args.label_tau, **hyper))
            then_hist = kickstart(col, kl, total_timesteps=steps, bc_coef=lambda i: args.bc_decay ** i,
                                  callback=show_then)
            print(f"kickstart: fused loss minibatches {kl.fused_updates} of {kl.n_updates}"
                  f" (masked: {kl.masked_fused_updates})")
        elif args.action_masks:
            mcol = RolloutCollector(env, pol, n_steps=args.n_steps, reward_norm=rnorm, action_masks=True)
            ml = timed_train(PPOLearner(pol, action_masks=True, **ppo_hyper))
            then_hist = learn(mcol, ml, total_timesteps=steps, callback=show_then)
            print(f"masked ppo: fused masked loss minibatches {ml.masked_fused_updates} of {ml.n_updates}")
        else:
            then_hist = learn(col, timed_train(PPOLearner(pol, **ppo_hyper)), total_timesteps=steps,
                              callback=show_then)
        torch.cuda.synchronize()
        then_s = time.time() - t1
        print(f"{args.then}: epochs run {sum(h['epochs_run'] for h in then_hist)} of "
              f"{args.then_iterations * args.epochs}, early stops {sum(bool(h['early_stop']) for h in then_hist)} of "
              f"{len(then_hist)} iterations, learner {learn_s[0]:.2f} s of {then_s:.2f} s")
        if args.action_masks:
            what = "masked warm start" if masked_imitation else "warm start"
            rows[f"{what}, then {args.then_iterations} x masked {args.then}, masked evaluation" + tag] = \
                evaluate_policy(pol, eval_rooms, action_masks=True, **kw)
            rows["the same policy, unmasked evaluation" + tag] = evaluate_policy(pol, eval_rooms, **kw)
        else:
            rows[f"warm start, then {args.then_iterations} x {args.then}" + tag] = evaluate_policy(pol, eval_rooms,
                                                                                                 **kw)
    env.close()
    rows["frontier planner"] = evaluate_planner(eval_rooms, **kw)
    print(f"warm start: {len(hist)} iterations, {hist[-1]['num_timesteps']} env steps, {train_s:.1f} s "
          f"(fused loss minibatches: {ln.fused_updates} of {ln.n_updates}, masked: {ln.masked_fused_updates})")
    print(RESULTS_HEADER)
    for label, r in rows.items():
        print(results_table_row(f"{args.eval_set}: {label}", r))
    print(json.dumps(dict(args=vars(args), train_seconds=train_s, history=hist, then_seconds=then_s,
                          then_learner_seconds=learn_s[0], then_history=then_hist,
                          table={k: {a: b for a, b in r.items() if a != "episodes"} for k, r in rows.items()})))


if __name__ == "__main__":
    main()
