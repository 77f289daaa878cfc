// Test driver (not part of the product): the host-only model compiler of csrc/model_build.h on a
// descriptor from a file, with no GPU and no HIP - g++ alone compiles it, which is the proof that
// the header is host-only (tests/test_model_build.py; by hand under -fsanitize=address,undefined).
// usage: model_build_check IN [OUT]
//   IN: a ps_task_cfg, then a ps_model_desc; optionally then int32 n_envs, int32 T, float
//   goal[T][89], int32 count[T] - with them every argument rule of ps_create runs (the keys and
//   fingers tables are not read by them), without them its hand_side rules only. Then
//   build_dev_model. Prints "<return code> <message>"; with OUT and code 0 writes the DevModel
//   bytes there. Exit status 0 whenever the input could be read.
#include <stdio.h>

#include <memory>
#include <string>
#include <vector>

#include "../diffusion-piano_amd/csrc/model_build.h"

using namespace ps;

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return fprintf(stderr, "usage: model_build_check IN [OUT]\n"), 2;
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
  }
  fclose(f);
  std::unique_ptr<DevModel> m(new DevModel);
  if (!rc) rc = build_dev_model(md.get(), m.get(), cfg.hand_side, err);
  printf("%d %s\n", rc, err.c_str());
  if (!rc && argc > 2) {
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(m.get(), sizeof(DevModel), 1, o) != 1 || fclose(o)) return fprintf(stderr, "cannot write\n"), 2;
  }
  return 0;
}
