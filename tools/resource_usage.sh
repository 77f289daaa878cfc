# Development aid: register / scratch / LDS use and spill counts of the step kernels'
# instantiations (pianosim_kernel<XG, WPE>, and pianosim_queue_kernel<XG>, the time-sliced step
# that launches of more than 2048 envs - the benchmark's - run), and the frames of the
# out-of-line narrow phases they call (x_pairs, x_refine: part of the caller's scratch), from the
# code object metadata and symbols of a device-only compile to assembly with the product flags
# (__graft_entry__._hipcc_lib); and, per kernel and out-of-line function, the static load figures of
# its assembly: the instructions in all and the v_mov / v_cndmask among them, the global_load and
# flat_load instructions (a flat_load is a read through a generic pointer: it takes the flat path
# and counts in both wait counters, where a typed LDS or global pointer gives ds_read /
# global_load), and the `s_waitcnt vmcnt` waits with exactly one global_load issued since the
# previous one (a model-table round trip paid on its own).
# usage: bash tools/resource_usage.sh [extra hipcc flags]
cd "$(dirname "$0")/.."
S=$(mktemp /tmp/ps_dev.XXXXXX.s)
trap 'rm -f "$S"' EXIT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value --cuda-device-only -S \
  -fno-hip-fp32-correctly-rounded-divide-sqrt -falign-loops=64 -mllvm -amdgpu-sched-strategy=max-ilp \
  "$@" -o "$S" diffusion-piano_amd/csrc/pianosim.hip || exit 1
awk '
  # out-of-line device functions: .set .L<symbol>.<field>, <value>
  /^[ \t]*\.set \.L_Z[0-9]+x_(pairs|refine)/ {
    split($2, a, "."); sym = a[2]; sub(/^L/, "", sym); f = a[3]; sub(/,$/, "", f)
    if (f == "num_vgpr") fv[sym] = $3
    if (f == "private_seg_size") { fs[sym] = $3; forder[++nf] = sym }
  }
  # the code of a kernel or function: from its label to its .Lfunc_end
  /^_Z[A-Za-z0-9_]+:/ { cur = $1; sub(/:$/, "", cur); since = 0 }
  /^\.Lfunc_end/ { cur = "" }
  cur != "" && /^[ \t]+(v|s|ds|flat|global|scratch|buffer)_[a-z0-9_]+/ { insts[cur]++ }
  cur != "" && /^[ \t]+v_mov_b/ { movs[cur]++ }
  cur != "" && /^[ \t]+v_cndmask/ { cnds[cur]++ }
  cur != "" && /^[ \t]+flat_load/ { flats[cur]++ }
  cur != "" && /^[ \t]+global_load/ { loads[cur]++; since++ }
  cur != "" && /^[ \t]+s_waitcnt.*vmcnt\(/ { waits[cur]++; if (since == 1) single[cur]++; since = 0 }
  # kernels: one amdhsa.kernels metadata entry each (its keys are sorted, .agpr_count first)
  /^  - \.agpr_count:/ { if (name != "") emit(); name = "-"; delete k }
  name != "" && /^    \.[a-z_]+:/ { key = $1; sub(/^\./, "", key); sub(/:$/, "", key); k[key] = $2; if (key == "name") name = $2 }
  /^  - \.agpr_count:/ { k["agpr_count"] = $3 }
  /^amdhsa\.target:/ { if (name != "") emit(); name = "" }
  function emit() {
    if (name !~ /pianosim_(queue_)?kernel|render_(scene|rays)_kernel/) return
    printf "%s\tVGPRs: %s\tAGPRs: %s\tSGPRs: %s\tScratchSize [bytes/lane]: %s\tVGPR spills: %s\tSGPR spills: %s\tLDS Size [bytes/block]: %s\n",
      name, k["vgpr_count"] - k["agpr_count"], k["agpr_count"], k["sgpr_count"], k["private_segment_fixed_size"],
      k["vgpr_spill_count"], k["sgpr_spill_count"], k["group_segment_fixed_size"]
    lorder[++nl] = name
  }
  END {
    for (i = 1; i <= nf; i++)
      printf "%s\t(out of line) VGPRs: %s\tframe [bytes/lane]: %s\n", forder[i], fv[forder[i]], fs[forder[i]]
    for (i = 1; i <= nf; i++) lorder[++nl] = forder[i]
    for (i = 1; i <= nl; i++)
      printf "%s\tinstructions: %d\tv_mov: %d\tv_cndmask: %d\tglobal_loads: %d\tflat_loads: %d\tvmcnt waits: %d\tvmcnt waits after a single global_load: %d\n",
        lorder[i], insts[lorder[i]], movs[lorder[i]], cnds[lorder[i]], loads[lorder[i]], flats[lorder[i]], waits[lorder[i]],
        single[lorder[i]]
  }' "$S"
