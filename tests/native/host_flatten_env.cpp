// host_flatten_env.cpp — host_flatten_power.cpp's C interface plus what PHX_LIGHT_INCLUDE_ENVIRONMENT adds to the flattened scene: the
// environment's direction tables (FlatScene::env_cdf: mcdf, then ccdf row by row), its interval of the selection table and the weight it
// entered that table with, for tests/test_environment_sampling.py.  Compiled with a plain host compiler beside csrc/scene_flatten.cpp.
#include "host_flatten_power.cpp"

extern "C" const void* hf_env_cdf(void* h, uint64_t* bytes) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  *bytes = fs.env_cdf.size() * sizeof(float);
  return fs.env_cdf.data();
}
extern "C" float hf_env_p(void* h) { return static_cast<Flat*>(h)->fs.env_p; }
extern "C" double hf_env_w(void* h) { return static_cast<Flat*>(h)->fs.env_w; }
