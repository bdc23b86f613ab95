// host_flatten_power.cpp — host_flatten.cpp's C interface plus the one array it does not export: the light selection table of
// PHX_LIGHT_SELECT_BY_POWER (FlatScene::light_pcdf), for tests/test_light_power.py.  Compiled with a plain host compiler beside
// csrc/scene_flatten.cpp, like the file it includes.
#include "host_flatten.cpp"

extern "C" const void* hf_power_table(void* h, uint64_t* bytes) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  *bytes = fs.light_pcdf.size() * sizeof(float);
  return fs.light_pcdf.data();
}
