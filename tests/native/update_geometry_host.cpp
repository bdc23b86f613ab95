// update_geometry_host.cpp — host_flatten.cpp's C interface plus flatten_geometry (csrc/scene_flatten.cpp) against the fingerprint of a
// committed scene, and the tables host_flatten.cpp does not export (the selection table, the environment's interval and weight), for
// tests/test_update_geometry.py.  Compiled with a plain host compiler beside csrc/scene_flatten.cpp, like the file it includes.
#include "host_flatten.cpp"

extern "C" {

// flatten `committed`, then flatten_geometry(`moved`) against its fingerprint -> a handle of host_flatten.cpp's kind (hf_status, hf_error,
// hf_array, hf_free); a `committed` that does not flatten gives its own status and message
void* hg_flatten_geometry(const phx_scene* committed, const phx_scene* moved, const phx_options* opt) {
  Flat* f = new Flat();
  FlatScene base;
  f->rc = flatten_scene(*committed, *opt, base, f->err);
  if (f->rc == PHX_OK) f->rc = flatten_geometry(*moved, *opt, base.fingerprint, f->fs, f->err);
  return f;
}
const void* hg_power_table(void* h, uint64_t* bytes) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  *bytes = fs.light_pcdf.size() * sizeof(float);
  return fs.light_pcdf.data();
}
// env_p's bits and env_w
void hg_environment(void* h, float* env_p, double* env_w) {
  const FlatScene& fs = static_cast<Flat*>(h)->fs;
  *env_p = fs.env_p; *env_w = fs.env_w;
}

}  // extern "C"
