#!/bin/bash
# rocprofv3 kernel stats of the bench modes (run on the MI355X box through gpurun, from the repo root):
#   tools/profile_modes.sh <tag> [sim] [cand] [hex] [mlp] [mlp_stable] [conv] [conv_all] [unet] [unet_all] [tasks_fixed] [tasks_random] [obst_fixed] [obst_random] [mlp_tasks_fixed] [mlp_tasks_random] [mlp_obst_fixed] [mlp_obst_random] [conv_tasks_fixed] [conv_tasks_random]     (*_all: every candidate row fed, --no_dedup)
# Writes gpurun_out/prof_<tag>_<mode>/ (trace + stats) and gpurun_out/prof_<tag>_<mode>.json (the bench line).
set -o pipefail
tag=$1; shift
root=$(pwd)
export TMPDIR=/tmp
for mode in "$@"; do
  out=$root/gpurun_out/prof_${tag}_${mode}
  case $mode in
    sim)  args="$root/bench.py --steps 100 --warmup 20 --no-cpu-baseline --no-other-modes" ;;
    cand) args="$root/bench.py --steps 60 --warmup 10 --no-cpu-baseline --no-other-modes --mode candidate-stability" ;;
    hex)  args="$root/bench.py --steps 60 --warmup 10 --no-cpu-baseline --no-other-modes --shapes hexagon --bridge_length 3" ;;
    mlp)  args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --tower 4 --max_steps 15 --model SuccessorMLP --loss mse_block_features" ;;
    mlp_stable) args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --tower 4 --max_steps 15 --model SuccessorMLP --loss mse_block_features --stable_actions_only" ;;
    conv) args="$root/tools/train_throughput.py --locksteps 4 --warmup 12 --envs 1024 --tower 2 --max_steps 10 --model ConvNet --loss mse_q_values" ;;
    conv_all) args="$root/tools/train_throughput.py --locksteps 4 --warmup 12 --envs 1024 --tower 2 --max_steps 10 --model ConvNet --loss mse_q_values --no_dedup" ;;
    unet) args="$root/tools/train_throughput.py --locksteps 3 --warmup 12 --envs 4096 --max_steps 15 --model UNet --loss mse_q_values+mse_block_features --shapes hexagon --bridge_length 3" ;;
    unet_all) args="$root/tools/train_throughput.py --locksteps 2 --warmup 3 --envs 4096 --max_steps 15 --model UNet --loss mse_q_values+mse_block_features --shapes hexagon --bridge_length 3 --no_dedup" ;;
    tasks_fixed)  args="$root/tools/random_task_throughput.py --tasks fixed3" ;;       # k_step / k_raster on three shared targets
    tasks_random) args="$root/tools/random_task_throughput.py --tasks random3" ;;      # + k_task_features, per-env k_step / k_raster
    obst_fixed)   args="$root/tools/random_task_throughput.py --random_obstacles 2 --tasks obst_fixed" ;;    # two shared obstacles: k_step / k_raster
    obst_random)  args="$root/tools/random_task_throughput.py --random_obstacles 2 --tasks obst_random" ;;   # RandomObstacles: + k_task_features (obstacle raster), k_raster reading env_obstacle_bits
    mlp_tasks_fixed)  args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --max_steps 15 --model SuccessorMLP --loss mse_block_features --fixed_targets 3" ;;
    mlp_tasks_random) args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --max_steps 15 --model SuccessorMLP --loss mse_block_features --random_targets 3" ;;   # per-row head, keyed groups, k_task_features in replay
    mlp_obst_fixed)  args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --max_steps 15 --model SuccessorMLP --loss mse_block_features --fixed_targets 3 --fixed_obstacles 2 --no_dedup" ;;
    mlp_obst_random) args="$root/tools/train_throughput.py --locksteps 6 --warmup 6 --envs 4096 --max_steps 15 --model SuccessorMLP --loss mse_block_features --random_targets 3 --random_obstacles 2" ;;   # k_bits_linear2, k_mlp_input<rows, obstacle bits>
    conv_tasks_fixed)  args="$root/tools/train_throughput.py --locksteps 4 --warmup 12 --envs 1024 --max_steps 10 --model ConvNet --loss mse_q_values --fixed_targets 3 --no_dedup" ;;
    conv_tasks_random) args="$root/tools/train_throughput.py --locksteps 4 --warmup 12 --envs 1024 --max_steps 10 --model ConvNet --loss mse_q_values --random_targets 3 --task_channels" ;;   # k_conv_input rows, rows keyed by task, per-transition rows in the captured step
    *) echo "unknown mode $mode"; exit 2 ;;
  esac
  (cd /tmp && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $out -- python3 $args) > $out.log 2>&1 || { tail -20 $out.log; exit 1; }
  grep "^{" $out.log | tail -1 > $out.json
  f=$(find $out -name "*kernel_stats.csv" | head -1)
  echo "== $mode: $f"; head -12 $f | cut -c1-200
  # keep the summaries, drop the raw trace (large)
  true
done
