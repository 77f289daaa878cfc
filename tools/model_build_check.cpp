// Test driver (not part of the product): the host-only model compiler of csrc/model_build.h on a
// descriptor from a file, with no GPU and no HIP - g++ alone compiles it, which is the proof that
// the header is host-only (tests/test_model_build.py; by hand under -fsanitize=address,undefined).
// usage: model_build_check IN [OUT [DIMS]]
//   IN: a ps_task_cfg, then a ps_model_desc; optionally then int32 n_envs, int32 T, float
//   goal[T][89], int32 count[T] - with them every argument rule of ps_create runs (the keys and
//   fingers tables are not read by them), without them its hand_side rules only. Then
//   build_dev_model and build_obs_extras. Prints "<return code> <message>"; with OUT and code 0
//   writes the DevModel bytes there, with DIMS (a third argument) the observation row as text:
//   the default part's width; the source codes of cfg.observables' extras (DevModel::obsx); the
//   extras' width for every mask 0 .. PS_OBS_ALL. Exit status 0 whenever the input could be read.
#include <stdio.h>

#include <memory>
#include <string>
#include <vector>

#include "../diffusion-piano_amd/csrc/model_build.h"

using namespace ps;

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return fprintf(stderr, "usage: model_build_check IN [OUT [DIMS]]\n"), 2;
  ps_task_cfg cfg;
  std::unique_ptr<ps_model_desc> md(new ps_model_desc);
  if (fread(&cfg, sizeof(cfg), 1, f) != 1 || fread(md.get(), sizeof(*md), 1, f) != 1)
    return fprintf(stderr, "short input\n"), 2;
  std::string err;
  int rc;
  int32_t head[2];
  if (fread(head, sizeof(head), 1, f) == 1) {  // the song: the whole of ps_create's argument rules
    const size_t T = head[1] > 0 ? (size_t)head[1] : 0;
    std::vector<float> goal(T * (NK + 1));
    std::vector<int32_t> count(T);
    if (T && (fread(goal.data(), sizeof(float), goal.size(), f) != goal.size() ||
              fread(count.data(), sizeof(int32_t), T, f) != T))
      return fprintf(stderr, "short song\n"), 2;
    const ps_song_desc song{head[1], goal.data(), count.data(), nullptr, nullptr};
    rc = check_create_args(md.get(), &song, &cfg, head[0], err);
  } else {
    rc = check_hand_side(md.get(), &cfg, err);
    if (!rc) rc = check_observables(&cfg, err);
  }
  fclose(f);
  std::unique_ptr<DevModel> m(new DevModel);
  if (!rc) rc = build_dev_model(md.get(), m.get(), cfg.hand_side, err);
  if (!rc) build_obs_extras(m.get(), cfg.observables, cfg.hand_side);
  if (!rc && argc > 3) {  // the handle's row, as ps_create computes it
    FILE* o = fopen(argv[3], "w");
    if (!o) return fprintf(stderr, "cannot write\n"), 2;
    fprintf(o, "%d\n", obs_base_dim(&cfg, m->n_obsj));
    for (int i = 0; i < m->n_obsx; i++) fprintf(o, "%d ", (int)m->obsx[i]);
    fprintf(o, "\n");
    std::unique_ptr<DevModel> w(new DevModel(*m));
    for (uint32_t mask = 0; mask <= PS_OBS_ALL; mask++) {
      build_obs_extras(w.get(), mask, cfg.hand_side);
      fprintf(o, "%d ", w->n_obsx);
    }
    if (fprintf(o, "\n") < 0 || fclose(o)) return fprintf(stderr, "cannot write\n"), 2;
  }
  printf("%d %s\n", rc, err.c_str());
  if (!rc && argc > 2) {
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(m.get(), sizeof(DevModel), 1, o) != 1 || fclose(o)) return fprintf(stderr, "cannot write\n"), 2;
  }
  return 0;
}
