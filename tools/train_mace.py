#!/usr/bin/env python3
"""Train a MACE policy end to end on the GPU (rollouts + trainer). Example (via gpurun):
   python tools/train_mace.py --arg-file args/opt_args_train_mace.txt --envs 4096 --frames 300"""
import argparse, os, sys
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before the HIP runtime starts (deepterrainrl_amd.configure_hw_queues)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deepterrainrl_amd import train_loop
ap = argparse.ArgumentParser()
ap.add_argument("--arg-file", default="args/opt_args_train_mace.txt")
ap.add_argument("--data-root", default=os.path.join(REPO, "tests", "golden", "refdata"))
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--iters", type=int, default=None)
ap.add_argument("--frames-per-drain", type=int, default=1)
ap.add_argument("--overlap", action="store_true", help="train on frame f while frame f+1 rolls out: frame f+1 is relaunched before frame f's tuples are drained (host-memory tuple rings), the weights are parked for the next launch (dog, native trainer, one GPU: 9.1 M sequential, 11.2-11.5 M overlapped; with round 2's PyTorch trainer it did not pay: 4.0 vs 4.7 M)")
ap.add_argument("--trainer", choices=["torch", "hip"], default="hip", help="hip: the MI355X-native trainer step (hip_trainer.py); torch: the PyTorch peer (trainer.py, HIP-graph replay)")
ap.add_argument("--reserve-cus", type=int, default=None, help="compute units per XCD kept out of the frame launches for the trainer's kernels (engine arg -reserve_cus=; default 0: measured 11.3 M env-steps/s without, 9.7 M with 2 per XCD -- the trainer's small GEMMs run 3x slower on 16-32 units than in the frame kernel's gaps on 256)")
ap.add_argument("--init-samples", type=int, default=None, help="override -trainer_num_init_samples= (the arg files collect 50 000 tuples before the first iteration: ~235 frames of 4096 dogs)")
ap.add_argument("--poll", action="store_true", help="with --overlap: relaunch env groups between Train() calls (dtrl_step_poll; measured: no gain on one GPU)")
ap.add_argument("--distributed", action="store_true", help="train_loop.train_distributed: sharded rollout + tuple gather to rank 0 + policy broadcast (RCCL). Start with torch.distributed.run for N ranks; alone it runs a one-rank RCCL group (DTRL_FORCE_COLLECTIVES=1), the config-3/4 loop shape on one GPU")
ap.add_argument("--data-parallel", action="store_true", help="with --distributed: no trainer rank -- every rank trains on its own tuples, gradients all-reduced (train_distributed(mode=\"data_parallel\"))")
ap.add_argument("--out", default=None, help="write weights (.npy) and <out>_scale.txt")
ap.add_argument("--variants", type=int, default=0, help="domain randomisation while training (train_loop.train(variants=...)): a table of this many model variants under seeded scales, every episode of every env under a model drawn afresh (0: off; not with --distributed)")
ap.add_argument("--variant-mass", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"), help="with --variants: range of the body-mass scale")
ap.add_argument("--variant-torque-lim", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"), help="with --variants: range of the torque-limit scale")
ap.add_argument("--variant-kp", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"), help="with --variants: range of the PD controllers' Kp scale")
ap.add_argument("--variant-kd", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"), help="with --variants: range of the PD controllers' Kd scale")
ap.add_argument("--variant-seed", type=int, default=0, help="with --variants: seed of the scales, the initial deal and the redraw")
ap.add_argument("--keep-nominal", type=float, default=None, help="with --variants: share of the draw's weight on the nominal model (default: 1 / variants)")
ap.add_argument("--rescale", action="store_true", help="continuous domain randomisation while training (train_loop.train(rescale=...)): every episode of every env under mass and motor scales drawn afresh on the device from --rescale-mass / -kp / -kd / -torque-lim (not with --distributed)")
for _q in ("mass", "kp", "kd", "torque-lim"):
    ap.add_argument("--rescale-" + _q, type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --rescale: range of the %s scale (default: not scaled)" % _q)
ap.add_argument("--rescale-per-link", nargs="*", default=[], choices=["mass", "kp", "kd", "torque_lim"], help="with --rescale: the quantities that draw one factor per link instead of one for all links")
ap.add_argument("--rescale-seed", type=int, default=0, help="with --rescale: seed of the draws")
ap.add_argument("--episode-limit", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="episode limits while training (train_loop.train(episode_limit=...)): every episode ends after LO .. HI frames at the latest, drawn per episode on the device, so that per-episode draws keep moving under a policy that no longer falls (not with --distributed)")
ap.add_argument("--episode-limit-seed", type=int, default=0, help="with --episode-limit: seed of the draws")
ap.add_argument("--episode-log", type=int, default=None, metavar="N", help="record every ended episode on the device (train_loop.train(episode_log=N): a ring of N rows per env group, drained with every log line): episodes, mean frames, mean distance and fall share per log interval (not with --distributed)")
ap.add_argument("--pushes", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="random pushes while training (train_loop.train(pushes=...)): every env is pushed on the device every LO .. HI frames (not with --distributed)")
ap.add_argument("--push-force", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --pushes: range of the force magnitude in N (default: the arg file's -min_perturb= / -max_perturb=)")
ap.add_argument("--push-duration", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --pushes: range of the duration in s (default: the arg file's)")
ap.add_argument("--push-seed", type=int, default=0, help="with --pushes: seed of the push streams")
ap.add_argument("--solver", default=None, choices=["sgd", "nesterov", "adagrad", "rmsprop", "adadelta", "adam"], help="Caffe solver type laid over the solver prototxt (train_loop.train(solver=...); default: what the file names, SGD where it names none; not with --distributed)")
ap.add_argument("--base-lr", type=float, default=None, help="with or without --solver: base_lr laid over the solver prototxt's")
ap.add_argument("--clip", type=float, default=None, help="clip_gradients: the gradient's L2 norm is scaled down to this where it exceeds it")
a = ap.parse_args()
solver = {k: v for k, v in (("type", a.solver), ("base_lr", a.base_lr), ("clip_gradients", a.clip)) if v is not None} or None
if solver and a.solver in ("adagrad", "rmsprop"):
    solver["momentum"] = 0.0       # (these two take none; the shipped files set 0.9 for SGD)
if solver and a.distributed:
    ap.error("--solver / --base-lr / --clip are not available with --distributed")
if a.pushes and a.distributed:
    ap.error("--pushes is not available with --distributed")
pushes = None
if a.pushes:
    pushes = dict(wait=tuple(a.pushes), seed=a.push_seed)
    if a.push_force:
        pushes["force"] = tuple(a.push_force)
    if a.push_duration:
        pushes["duration"] = tuple(a.push_duration)
if a.variants and a.distributed:
    ap.error("--variants is not available with --distributed")
if a.rescale and a.distributed:
    ap.error("--rescale is not available with --distributed")
if a.episode_limit and a.distributed:
    ap.error("--episode-limit is not available with --distributed")
episode_limit = dict(frames=tuple(a.episode_limit), seed=a.episode_limit_seed) if a.episode_limit else None
if a.episode_log is not None and a.distributed:
    ap.error("--episode-log is not available with --distributed")
rescale = None
if a.rescale:
    rescale = dict(seed=a.rescale_seed, per_link=tuple(a.rescale_per_link))
    for _q in ("mass", "kp", "kd", "torque_lim"):
        if getattr(a, "rescale_" + _q) is not None:
            rescale[_q] = tuple(getattr(a, "rescale_" + _q))
variants = None
if a.variants:
    variants = dict(count=a.variants, mass=tuple(a.variant_mass), torque_lim=tuple(a.variant_torque_lim), kp=tuple(a.variant_kp), kd=tuple(a.variant_kd), seed=a.variant_seed)
    if a.keep_nominal is not None:
        variants["keep_nominal"] = a.keep_nominal
reserve = a.reserve_cus if a.reserve_cus is not None else (1 if (a.distributed and not a.data_parallel) else 0)   # (the exchange's collective and read-backs beside the rollout: 11.0 M with one unit per XCD set aside, 9.6 M without)
if a.distributed:
    import torch, torch.distributed as dist
    os.environ.setdefault("DTRL_FORCE_COLLECTIVES", "1")
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29541"), ("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        os.environ.setdefault(k, v)
    lr = int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(lr)
    dist.init_process_group(backend="nccl", device_id=torch.device("cuda", lr))
    world = dist.get_world_size()
    ea = dict(({"trainer_num_init_samples": a.init_samples} if a.init_samples is not None else {}), **({"reserve_cus": reserve} if reserve else {})) or None
    st = train_loop.train_distributed(a.arg_file, a.data_root, a.envs * world, dist, max_iters=a.iters, max_frames=a.frames, extra_args=ea, device="cuda:%d" % lr,
                                      trainer_device="cuda:%d" % lr, local_device_id=lr, trainer=a.trainer, overlap=a.overlap, mode="data_parallel" if a.data_parallel else "gather")
    if dist.get_rank() == 0:
        print("[distributed x%d%s, trainer=%s, overlap=%s] frames %d  trainer iters %d  tuples %d  %.1f s  ->  %.2f M env-steps/s while training (all ranks), %.1f trainer iters/s" % (
            world, " data-parallel" if a.data_parallel else "", a.trainer, a.overlap, st["frames"], st["iters"], st["tuples"], st["seconds"], st["env_steps_per_s"] / 1e6, st["iters"] / st["seconds"]))
        if "phases" in st:
            print("   [distributed] rank 0 host wall-clock by phase (ms per frame): " + "  ".join("%s %.2f" % (k, 1e3 * v / max(st["frames"], 1)) for k, v in st["phases"].items()))
    dist.barrier(); dist.destroy_process_group()
    sys.exit(0)
st = train_loop.train(a.arg_file, a.data_root, a.envs, max_iters=a.iters, max_frames=a.frames, log_every=50, overlap=a.overlap, frames_per_drain=a.frames_per_drain,
                      extra_args=dict(({"reserve_cus": reserve} if reserve else {}), **({"trainer_num_init_samples": a.init_samples} if a.init_samples is not None else {})) or None,
                      out_scale_file=(a.out + "_scale.txt") if a.out else None, trainer=a.trainer, poll=a.poll, variants=variants, pushes=pushes, solver=solver, rescale=rescale, episode_limit=episode_limit, episode_log=a.episode_log)
if a.episode_log is not None:
    print("[episode log] %(episodes)d episodes, %(frames)d frames, %(falls)d ended by a fall, %(lost)d rows lost" % st["episode_log"])
if episode_limit:
    print("[episode limit] %d .. %d frames; %d episodes ended by the limit, %d by a fall" % (a.episode_limit[0], a.episode_limit[1], int(st["episode_limit"]["by_limit"].sum()), int(st["episode_limit"]["by_fall"].sum())))
if a.out:
    np.save(a.out + ".npy", st["weights"])
if variants:
    print("[variants] %d models, %d draws; envs per variant at the end: %s" % (a.variants, int(st["variants"]["draws"].sum()), np.bincount(st["variants"]["variant"], minlength=a.variants).tolist()))
if rescale:
    print("[rescale] %d episode starts under drawn scales, most on one env %d" % (int(st["rescale"]["episodes"].sum()), int(st["rescale"]["episodes"].max())))
if pushes:
    print("[pushes] every %d .. %d frames; %d pushes, most on one env %d" % (a.pushes[0], a.pushes[1], int(st["pushes"]["pushes"].sum()), int(st["pushes"]["pushes"].max())))
print("[trainer=%s reserve_cus=%d side-stream start delay %.0f us] " % (a.trainer, reserve, st["side_stream_delay_us"]), end="")
print("frames %d  trainer iters %d  tuples %d  %.1f s  ->  %.2f M env-steps/s while training, %.1f trainer iters/s" % (
    st["frames"], st["iters"], st["tuples"], st["seconds"], st["env_steps_per_s"] / 1e6, st["trainer_iters_per_s"]))
print("   host wall-clock by phase (ms per frame): " + "  ".join("%s %.2f" % (k, 1e3 * v / max(st["frames"], 1)) for k, v in st["phases"].items() if k != "early_relaunches") + "  | env groups relaunched between Train() calls: %d" % st["phases"].get("early_relaunches", 0))
