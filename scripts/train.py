#!/usr/bin/env python3
"""ControlNet / LoRA training launcher on the MI355X training step — mirror of the reference's scripts/train/train.py: the SAME command
line (`wan_parser`, src/goal_force/utils.py:854-900), dataset mux (train.py:126-197), training module (train.py:12-124: load the
models, freeze all but `--trainable_models controlnet`, scheduler in training mode, trainable LoRA adapters on `--lora_base_model`
(`--lora_target_modules`, `--lora_rank`, `--lora_checkpoint`; utils.py:569-584), optional `--controlnet_checkpoint`) and loop
(`launch_training_task`, utils.py:734-826).  One process per GPU: where the reference starts `accelerate launch` with a DeepSpeed
ZeRO-2 config, start this with `python -m torch.distributed.run --nproc-per-node N scripts/train.py ...` (gradients are averaged over
RCCL, goal_force_amd/training.py::allreduce_gradients; 288 GB of HBM hold the frozen expert, the ControlNet, its fp32 moments and the
activations of an 81-frame item without ZeRO or offload).

    python scripts/train.py --dataset_base_path balls dominos plants --dataset_metadata_path balls.csv dominos.csv plants.csv \\
        --control_signal_type direct_force_and_goal_force_and_mass --controlnet_num_layers 10 --height 480 --width 832 --num_frames 81 \\
        --model_paths '["...high_noise_model shards...", "models_t5_umt5-xxl-enc-bf16.pth", "Wan2.1_VAE.pth"]' --learning_rate 1e-5 \\
        --num_epochs 2 --save_steps 500 --trainable_models controlnet --extra_inputs input_image --max_timestep_boundary 0.358 \\
        --max_grad_norm 1 --p_mask_out_masses 0.5 --p_mask_out_direct_force 0.5 --p_mask_out_indirect_force 0.5

Clips are decoded by cv2 as in the reference when it is importable; this image has neither cv2 nor imageio, so clips may also be
directories of frame images or `.npy` files (goal_force_amd/force_map.py::load_video_frames)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

MODELS = "./models/Wan-AI"


def model_configs(args):
    """parse_model_configs / parse_model_configs_offline (utils.py:495-530): `--model_paths` is a JSON list of files or shard lists;
    `--model_id_with_origin_paths "id:pattern,..."` resolves under ./models/<id>/<pattern> (no downloads here)."""
    from goal_force_amd.pipeline import ModelConfig
    cfgs = []
    if args.model_paths is not None:
        cfgs += [ModelConfig(path=p) for p in json.loads(args.model_paths)]
    if args.model_id_with_origin_paths is not None:
        for item in args.model_id_with_origin_paths.split(","):
            mid, pattern = item.split(":")
            cfgs.append(ModelConfig(model_id=mid, origin_file_pattern=pattern))
    return cfgs


def check_args(args):
    """What the HIP training step differentiates: the ControlNet (`--trainable_models controlnet`), LoRA adapters on one model's
    blocks (`--lora_base_model dit`; `--trainable_models` may then be empty), or both.  Needs no device."""
    if args.apply_strided_controlnet or args.controlnet_stride is not None:
        raise NotImplementedError("strided ControlNet is not used by Goal Force")
    if args.control_signal_type not in ("canny_edge", "direct_force_and_goal_force_and_mass"):
        raise NotImplementedError(args.control_signal_type)                                            # train.py:33-38
    trainable = args.trainable_models or ""
    if getattr(args, "enable_fp8_training", False):
        # the experts' blocks run fp8 and frozen (training.set_fp8_frozen: dX on the fp8 GEMM, no weight gradient); nothing of them may train
        if args.lora_base_model is not None and not getattr(args, "lora_beside_fp8", False):
            raise NotImplementedError("--enable_fp8_training: trainable LoRA adapters run on bf16 layers only (the fp8 tape is open to frozen "
                                      "blocks: drop --lora_base_model)")
        if any(m in ("dit", "dit2") for m in trainable.split(",")):
            raise NotImplementedError("--enable_fp8_training: the experts run fp8 and frozen: --trainable_models may not name dit or dit2")
    if args.lora_base_model is None:
        if args.lora_checkpoint is not None:
            raise NotImplementedError("--lora_checkpoint needs --lora_base_model (the reference ignores it without one; here it is an error)")
        if trainable != "controlnet":
            raise NotImplementedError("--trainable_models controlnet is what the HIP training step differentiates")
    else:
        if args.lora_base_model not in ("dit", "dit2", "controlnet"):
            raise NotImplementedError(f"--lora_base_model {args.lora_base_model}: adapters train on the blocks of dit, dit2 or controlnet")
        if trainable not in ("", "controlnet"):
            raise NotImplementedError("--trainable_models: empty or controlnet beside --lora_base_model")
        if not 1 <= args.lora_rank <= 256:
            raise NotImplementedError(f"--lora_rank {args.lora_rank}: expected 1 <= r <= 256")


def add_lora(pipe, args):
    """switch_pipe_to_training_mode's LoRA part (utils.py:569-584): inject trainable adapters into `--lora_base_model` (after the
    freeze, so only they and `--trainable_models` train), then optionally restore them from `--lora_checkpoint`."""
    if args.lora_base_model is None:
        return 0
    from goal_force_amd import lora
    if getattr(args, "lora_beside_fp8", False):
        lora.set_beside_fp8(True)      # before the adapters exist: they go beside Linears that carry (or will carry) an fp8 copy
    from goal_force_amd.checkpoints import load_state_dict
    model = getattr(pipe, args.lora_base_model, None)
    if model is None:
        raise NotImplementedError(f"--lora_base_model {args.lora_base_model}: the pipeline holds no such model")
    n = lora.add_trainable(model, args.lora_target_modules.split(","), args.lora_rank)
    if args.lora_checkpoint is not None:
        lora.load_trainable_state(model, load_state_dict(args.lora_checkpoint), source=args.lora_checkpoint)
    return n


def parser():
    """wan_parser (the reference's command line, pinned argument for argument) plus `--enable_fp8_training`, which the reference passes
    to its training module rather than its parser (train.py:42, 51, 62: computation in float8_e4m3fn over the frozen base)."""
    from goal_force_amd.training import wan_parser
    ap = wan_parser()
    ap.add_argument("--enable_fp8_training", default=False, action="store_true",
                    help="Run the frozen experts' blocks on the fp8 kernels, forward and backward (ControlNet training only).")
    ap.add_argument("--lora_beside_fp8", default=False, action="store_true",
                    help="With --enable_fp8_training: train the --lora_base_model adapters beside the frozen fp8 Linears (lora.set_beside_fp8).")
    return ap


def enable_fp8_training(pipe, args):
    """`--enable_fp8_training`: enable_fp8 on both experts (frozen by freeze_except: check_args lets no expert train beside the flag)
    and the tape opened to frozen fp8 blocks.  -> the number of experts switched."""
    if not getattr(args, "enable_fp8_training", False):
        return 0
    from goal_force_amd import dit, training
    experts = [m for m in (getattr(pipe, "dit", None), getattr(pipe, "dit2", None)) if m is not None]
    for m in experts:
        dit.enable_fp8(m)
    training.set_fp8_frozen(True)
    return len(experts)


class WanTrainingModule:
    """train.py:12-124 around the HIP pipeline: what launch_training_task needs of it (`.pipe`, `.extra_inputs`, the timestep
    boundaries)."""

    def __init__(self, args, device):
        import torch
        from goal_force_amd.pipeline import ModelConfig, WanVideoPipeline
        check_args(args)
        self.pipe = WanVideoPipeline.from_pretrained(
            torch_dtype=torch.bfloat16, device=device, model_configs=model_configs(args), controlnet=True,
            controlnet_num_layers=args.controlnet_num_layers,
            tokenizer_config=ModelConfig(model_id="Wan-AI/Wan2.1-T2V-1.3B", origin_file_pattern="google/*",
                                         path=f"{MODELS}/Wan2.1-T2V-1.3B/google/umt5-xxl"))               # train.py:43-55
        self.pipe.scheduler.set_timesteps(1000, training=True)                                             # utils.py:560
        self.pipe.freeze_except([] if args.trainable_models is None else args.trainable_models.split(","))   # utils.py:563
        add_lora(self.pipe, args)                                                                          # utils.py:569-584
        enable_fp8_training(self.pipe, args)
        if args.controlnet_checkpoint is not None:                                                        # utils.py:586-590
            self.pipe.load_controlnet_weights(self.pipe.controlnet, args.controlnet_checkpoint, torch_dtype=torch.bfloat16)
            print(f"ControlNet checkpoint loaded: {args.controlnet_checkpoint}, total {len(self.pipe.controlnet.state_dict())} keys")
        else:
            print("No ControlNet checkpoint provided. Starting training from scratch.")
        self.extra_inputs = args.extra_inputs.split(",") if args.extra_inputs is not None else []
        self.max_timestep_boundary, self.min_timestep_boundary = args.max_timestep_boundary, args.min_timestep_boundary


def main(argv=None):
    from goal_force_amd import training as tr
    args = parser().parse_args(argv)
    import torch
    from goal_force_amd.distributed import init_from_env
    rank, local, world = init_from_env()
    torch.cuda.set_device(local)
    if world > 1 and "OMP_NUM_THREADS" not in os.environ:
        torch.set_num_threads(max(1, min(16, (os.cpu_count() or 8) // world)))
    device = torch.device("cuda", local)
    dataset = tr.get_dataset(args, device=device)                          # (launch_training_task shards it over the ranks, as accelerator.prepare does)
    model = WanTrainingModule(args, device)
    log = (lambda rec, step: print(f"[step {step}] " + ", ".join(f"{k} {v:.6g}" for k, v in rec.items()), flush=True)) if rank == 0 else None
    tr.launch_training_task(dataset, model, args=args, log=log)


if __name__ == "__main__":
    main()
