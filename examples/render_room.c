/* A host written in plain C against include/phx_xpu.h — the same call sequence the reference's session_t::render makes
 * through xpu_t (plugins/blender/session.cpp:73-94: discover -> preprocess -> tiles_t::make -> start -> join), with no
 * Python, no C++ and no torch in the process.  Renders a small room (floor, back wall, emissive ceiling panel, two
 * tilted triangles) and writes the raw fp32 film (H x W x 4) to argv[1].
 *   make -C examples
 *   ./render_room film.f32 [host-bvh|device-bvh|auto-bvh] [N] [area-lights|power-lights|sample-environment] [error-estimate] [adaptive TAU] [denoise|denoise-guided] [progressive K [tiles TAU]] [display [auto]] [despeckle] [orbit K [clamp]]
 * area-lights (anywhere behind the film's name): next-event estimation picks a light's triangle by area (PHX_LIGHTS_BY_AREA) instead of by
 * index as the reference does; the room's panel is two equal triangles, so the film is the same.
 * power-lights: that, and the light itself by power instead of uniformly (PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER); the room has one
 * light, so the film is the same again.
 * sample-environment: the room gets a sky -- an environment material with a small lat-long image, dim but for one bright texel -- and next-event
 * estimation samples it beside the panel (PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER | PHX_LIGHT_INCLUDE_ENVIRONMENT).
 * error-estimate: the frame asks for the per-pixel error estimate (phx_frame.moments_channel: 3 more floats per pixel, the centred second
 * moment of the pixel's samples) and the host prints the film's mean relative standard error; the file written stays H x W x 4, the same floats.
 * adaptive TAU: adaptive sampling (phx_dev_set_adaptive) with threshold TAU, a first decision after 4 of the 8 samples and one every 2 from there
 * on: a pixel stops once the standard error of its extrapolated value is at most TAU times the value.  The frame carries the error estimate
 * and one more float per pixel, the samples the pixel took; the host prints their mean.  The file written stays H x W x 4.
 * denoise: the joined film goes through the film denoiser (phx_dev_denoise, 5 iterations, sigma_l 4; the film has no normals channel, so the
 * filter is guided by luminance alone) in place before it is written; the frame carries the error estimate, which is the filter's yardstick,
 * and the host prints the mean of the m2 channel before and after.  Without the keyword nothing of this runs.
 * denoise-guided: the same, guided by the first hit's albedo: the host renders the guide film of the frame's seed (phx_dev_render_guides, 4 samples a
 * pixel) and hands it to phx_dev_denoise_guided with PHX_GUIDE_DEMODULATE (the film has no normals channel, which PHX_GUIDE_PLANE would need).
 * progressive K: K frames of 8 samples at seeds 7, 8, ... are pooled into one accumulator film (phx_dev_film_accumulate: primary rgba, m2 rgb, samples),
 * each frame carrying the error estimate; after every frame the host prints the call's summary (the samples pooled so far and the pixels whose
 * standard error is at most 0.05 * (|value| + 0.01)).  The accumulator is what the later steps (denoise) see and what is written.
 * progressive K tiles TAU: the same, but from the second frame on a frame renders only the 32 x 32 tiles that phx_dev_film_tile_map of the
 * accumulator leaves open at the threshold TAU (floor 0.01), through a queue of phx_tiles_make_list; the frame films carry "samples", so the
 * pooling leaves the pixels of a tile that was not rendered alone.  Per frame the host prints `tiles: frame k open O of T rendered P pixels`,
 * and it stops early once no tile is open.
 * display [auto]: after every other step the film at hand goes through the display pass (phx_dev_film_display: exposure 1, or with `auto` taken from
 * the film's own luminance histogram so that its logarithmic mean between the 50th and 95th percentile lands on 0.18; the ACES curve, the sRGB
 * transfer function, ordered dither) and the 8-bit image is written to argv[1] + ".ppm"; the host prints the scale and the call's counters.
 * orbit K: instead of the steps above, K cameras on an arc about the room's middle, one frame of 8 samples each at seeds 7, 8, ... on ONE device that
 * preprocessed once: per camera phx_dev_set_camera, the guide film (phx_dev_render_guides), from the second camera on phx_dev_film_reproject of the
 * accumulator (the host prints its summary), the frame, phx_dev_film_accumulate and the display pass into argv[1] + ".orbit<k>.ppm" (DESIGN 22).
 * The last accumulator is what is written to argv[1].
 * orbit K clamp: that, and from the second camera on the reprojected accumulator is clamped against the neighbourhoods of this camera's frame film
 * before the frame is pooled (phx_dev_film_outlier_clamp: radius 1, two-sided, the centre included, gamma 3, a clamped pixel claims at most 8 samples;
 * DESIGN 23); the host prints the call's summary.
 * despeckle: every joined frame film is clamped in place against its own neighbourhoods before anything else reads it (phx_dev_film_outlier_clamp:
 * radius 2, the centre excluded, upper only, gamma 4, the 2 brightest taps left out); the frame carries the error estimate, which is scaled with a
 * clamped colour, and the host prints the call's summary.  The clamp is biased: what the fireflies carried is gone from the film.
 * With N > 1 it is the reference's multi-device mechanism (src/core.cpp:103-115): N devices — one per GPU that phx_discover
 * reports, wrapping around when the box has fewer — are all started on ONE tile queue and ONE film, and joined in turn.
 * No collective: whoever renders a tile writes it into the shared film.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phx_xpu.h"

#define W 128
#define H 96

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, phx_last_error());
  return 1;
}

/* orbit K on a device that has preprocessed `scene`: see the head of the file.  Frames carry normals and the error estimate (10 floats a pixel),
 * the accumulator also "samples" (11): the layouts phx_reproject reads. */
static int orbit(phx_device* dev, const phx_scene* scene, const phx_options* opt, int count, int clamp, const char* path) {
  const size_t xf = 10, xa = 11, npix = (size_t)W * H;
  float* film = (float*)calloc(npix * xf, sizeof(float));
  float* acc = (float*)calloc(npix * xa, sizeof(float));
  float* next = (float*)calloc(npix * xa, sizeof(float));
  float* guides[2] = {(float*)calloc(npix * 8, sizeof(float)), (float*)calloc(npix * 8, sizeof(float))};
  uint8_t* image = (uint8_t*)malloc(npix * 4);
  char* name = (char*)malloc(strlen(path) + 32);
  phx_tiles* tiles = phx_tiles_make(W, H, 32, 0, 1);
  if (!film || !acc || !next || !guides[0] || !guides[1] || !image || !name || !tiles) return 1;
  phx_camera before = scene->camera;
  for (int k = 0; k < count; ++k) {
    phx_camera cam = scene->camera; /* on an arc about (0, 0, -3), looking at it: rows of to_world are the camera's axes, then its origin */
    const float a = 0.08f * (float)k, c = cosf(a), s = sinf(a);
    memset(cam.to_world, 0, sizeof(cam.to_world));
    cam.to_world[0] = c; cam.to_world[2] = -s; cam.to_world[5] = 1.0f; cam.to_world[8] = s; cam.to_world[10] = c; cam.to_world[15] = 1.0f;
    cam.to_world[12] = 3.0f * s; cam.to_world[14] = -3.0f + 3.0f * c;
    if (phx_dev_set_camera(dev, &cam) != PHX_OK) return fail("phx_dev_set_camera");
    phx_guides gp;
    memset(&gp, 0, sizeof(gp));
    gp.sampler_seed = 7 + (uint64_t)k; gp.samples = 4;
    if (phx_dev_render_guides(dev, &gp, guides[k & 1]) != PHX_OK) return fail("phx_dev_render_guides");
    if (k > 0) { /* carry the accumulator to this camera */
      phx_reproject rp;
      phx_reproject_summary rs;
      memset(&rp, 0, sizeof(rp));
      rp.width = W; rp.height = H; rp.xstride_a = (uint32_t)xa; rp.normals_offset_a = 4; rp.m2_offset_a = 7; rp.samples_offset_a = 10; rp.xstride_g = 8;
      rp.from = before; rp.to = cam; rp.sigma_plane = 1.0f; rp.sigma_dist = 4.0f; rp.max_history = 64;
      if (phx_dev_film_reproject(dev, &rp, acc, guides[(k - 1) & 1], guides[k & 1], next, &rs) != PHX_OK) return fail("phx_dev_film_reproject");
      printf("orbit: camera %d reused %llu no_geometry %llu disoccluded %llu of %llu samples %llu\n", k + 1, (unsigned long long)rs.reused,
             (unsigned long long)rs.no_geometry, (unsigned long long)rs.disoccluded, (unsigned long long)rs.pixels, (unsigned long long)rs.samples);
      float* t = acc; acc = next; next = t;
    }
    phx_frame frame;
    memset(&frame, 0, sizeof(frame));
    memset(film, 0, npix * xf * sizeof(float));
    phx_tiles_reset(tiles);
    frame.tiles_user = tiles; frame.next_tile = phx_tiles_next; frame.sampler_seed = 7 + (uint64_t)k; frame.primary_components = 4;
    frame.normals_channel = 1; frame.moments_channel = 1; frame.host_film = film;
    if (phx_dev_start(dev, &frame) != PHX_OK) return fail("phx_dev_start");
    if (phx_dev_join(dev) != PHX_OK) return fail("phx_dev_join");
    if (clamp && k > 0) { /* the history against what this camera's first frame shows, before that frame is pooled into it */
      phx_outlier_clamp oc;
      phx_outlier_clamp_summary os;
      memset(&oc, 0, sizeof(oc));
      oc.width = W; oc.height = H; oc.xstride_a = (uint32_t)xa; oc.m2_offset_a = 7; oc.samples_offset_a = 10; oc.xstride_b = (uint32_t)xf;
      oc.radius = 1; oc.trim = 0; oc.min_taps = 4; oc.gamma = 3.0f; oc.clamped_history = 8;
      if (phx_dev_film_outlier_clamp(dev, &oc, acc, film, acc, &os) != PHX_OK) return fail("phx_dev_film_outlier_clamp");
      printf("orbit: camera %d clamped %llu capped %llu inside %llu skipped %llu unbounded %llu of %llu\n", k + 1, (unsigned long long)os.clamped,
             (unsigned long long)os.capped, (unsigned long long)os.inside, (unsigned long long)os.skipped, (unsigned long long)os.unbounded,
             (unsigned long long)os.pixels);
    }
    phx_accumulate pa;
    memset(&pa, 0, sizeof(pa));
    pa.width = W; pa.height = H; pa.xstride_a = (uint32_t)xa; pa.normals_offset_a = 4; pa.m2_offset_a = 7; pa.samples_offset_a = 10;
    pa.xstride_b = (uint32_t)xf; pa.normals_offset_b = 4; pa.m2_offset_b = 7; pa.spp_b = opt->samples_per_pixel;
    if (phx_dev_film_accumulate(dev, &pa, acc, film, NULL) != PHX_OK) return fail("phx_dev_film_accumulate");
    phx_display dp;
    memset(&dp, 0, sizeof(dp));
    dp.width = W; dp.height = H; dp.xstride = (uint32_t)xa; dp.flags = PHX_DISPLAY_DITHER; dp.tone = PHX_TONE_ACES; dp.scale = 1.0f;
    dp.key = 0.18f; dp.low_q16 = 32768; dp.high_q16 = 62259; dp.min_scale = 1.0f / 4096.0f; dp.max_scale = 4096.0f;
    if (phx_dev_film_display(dev, &dp, acc, image, NULL, NULL) != PHX_OK) return fail("phx_dev_film_display");
    sprintf(name, "%s.orbit%d.ppm", path, k + 1);
    FILE* f = fopen(name, "wb");
    int ok = f != NULL && fprintf(f, "P6\n%d %d\n255\n", W, H) > 0;
    for (size_t p = 0; ok && p < npix; ++p) ok = fwrite(image + 4 * p, 1, 3, f) == 3; /* alpha is dropped */
    if (!ok) { fprintf(stderr, "cannot write %s\n", name); return 1; }
    fclose(f);
    before = cam;
  }
  FILE* f = fopen(path, "wb");
  int ok = f != NULL;
  for (size_t p = 0; ok && p < npix; ++p) ok = fwrite(acc + p * xa, sizeof(float), 4, f) == 4;
  if (!ok) { fprintf(stderr, "cannot write %s\n", path); return 1; }
  fclose(f);
  phx_tiles_free(tiles);
  free(film); free(acc); free(next); free(guides[0]); free(guides[1]); free(image); free(name);
  return 0;
}

/* `animate K`: the two tilted triangles (vertices 12 .. 17) slide along x over K frames.  Every frame the host hands the moved vertices to
 * phx_dev_update_geometry (a refit: the tree keeps its topology), prints what the update cost and renders one fresh film;
 * nothing is accumulated across geometry.  The last film is written to `path`. */
static int animate(phx_device* dev, phx_scene* scene, phx_mesh* mesh, int frames, const char* path) {
  float moved[54];
  const float* rest = mesh->vertices;
  if (mesh->num_vertices != 18) { fprintf(stderr, "animate: the room's mesh has 18 vertices, not %u\n", mesh->num_vertices); return 1; }
  float* film = (float*)calloc((size_t)W * H * 4, sizeof(float));
  if (!film) return 1;
  for (int k = 1; k <= frames; ++k) {
    memcpy(moved, rest, sizeof(moved));
    for (int v = 12; v < 18; ++v) moved[3 * v] = rest[3 * v] + 0.8f * (float)k / (float)frames;
    mesh->vertices = moved;
    phx_geometry_update u;
    memset(&u, 0, sizeof(u));
    u.mode = PHX_UPDATE_REFIT;
    phx_geometry_summary gs;
    if (phx_dev_update_geometry(dev, scene, &u, &gs) != PHX_OK) { mesh->vertices = rest; free(film); return fail("phx_dev_update_geometry"); }
    double ms[4];
    if (phx_dev_update_geometry_times(dev, ms) != PHX_OK) { mesh->vertices = rest; free(film); return fail("phx_dev_update_geometry_times"); }
    printf("update: frame %d refit %.3f ms\n", k, ms[3]);
    phx_tiles* tiles = phx_tiles_make(W, H, 32, 0, 1);
    phx_frame frame;
    memset(&frame, 0, sizeof(frame));
    frame.tiles_user = tiles; frame.next_tile = phx_tiles_next;
    frame.sampler_seed = 7; frame.primary_components = 4; frame.host_film = film;
    const int bad = phx_dev_start(dev, &frame) != PHX_OK || phx_dev_join(dev) != PHX_OK;
    phx_tiles_free(tiles);
    if (bad) { mesh->vertices = rest; free(film); return fail("phx_dev_start / phx_dev_join"); }
    printf("animate: frame %d triangles %u nodes %u levels %u bounds x %.3f .. %.3f\n", k, gs.triangles, gs.nodes, gs.levels, (double)gs.bounds[0], (double)gs.bounds[3]);
  }
  mesh->vertices = rest;
  FILE* f = fopen(path, "wb");
  const int ok = f != NULL && fwrite(film, sizeof(float), (size_t)W * H * 4, f) == (size_t)W * H * 4;
  if (f) fclose(f);
  free(film);
  if (!ok) { fprintf(stderr, "cannot write %s\n", path); return 1; }
  return 0;
}

/* despeckle: a joined frame film of `xstride` floats a pixel (primary rgba, m2 rgb [, samples]) against its own neighbourhoods, in place */
static int despeckle_film(phx_device* dev, float* film, size_t xstride, int has_samples, int frame_number) {
  phx_outlier_clamp oc;
  phx_outlier_clamp_summary os;
  memset(&oc, 0, sizeof(oc));
  oc.width = W; oc.height = H; oc.xstride_a = oc.xstride_b = (uint32_t)xstride; oc.m2_offset_a = 4; oc.samples_offset_a = has_samples ? 7 : 0;
  oc.flags = PHX_OUTLIER_EXCLUDE_CENTRE | PHX_OUTLIER_UPPER_ONLY; oc.radius = 2; oc.trim = 2; oc.min_taps = 4; oc.gamma = 4.0f;
  double before = 0.0, after = 0.0;
  for (size_t p = 0; p < (size_t)W * H; ++p) for (int c = 0; c < 3; ++c) before += film[p * xstride + c];
  if (phx_dev_film_outlier_clamp(dev, &oc, film, film, film, &os) != PHX_OK) return fail("phx_dev_film_outlier_clamp");
  for (size_t p = 0; p < (size_t)W * H; ++p) for (int c = 0; c < 3; ++c) after += film[p * xstride + c];
  printf("despeckle: frame %d clamped %llu inside %llu skipped %llu unbounded %llu of %llu film mean %.6g -> %.6g\n", frame_number, (unsigned long long)os.clamped,
         (unsigned long long)os.inside, (unsigned long long)os.skipped, (unsigned long long)os.unbounded, (unsigned long long)os.pixels,
         before / (3.0 * W * H), after / (3.0 * W * H));
  return 0;
}

int main(int argc, char** argv) {
  static const float vertices[] = {
      /* floor y = -1 */ -2, -1, -1, 2, -1, -1, 2, -1, -5, -2, -1, -5,
      /* back wall z = -5 */ -2, -1, -5, 2, -1, -5, 2, 2, -5, -2, 2, -5,
      /* ceiling panel y = 1.5, facing down */ -1, 1.5f, -2, -1, 1.5f, -4, 1, 1.5f, -4, 1, 1.5f, -2,
      /* two tilted triangles */ -0.8f, -0.9f, -3.2f, 0.9f, -0.6f, -3.6f, 0.1f, 0.7f, -3.0f, -1.5f, -0.2f, -4.2f, -0.6f, 0.9f, -4.4f, -1.7f, 1.1f, -3.9f};
  static const uint32_t faces[] = {0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7, 8, 9, 10, 8, 10, 11, 12, 13, 14, 15, 16, 17};
  static const uint32_t grey_faces[] = {0, 1, 2, 3}, light_faces[] = {4, 5}, red_faces[] = {6, 7};

  phx_material materials[4]; /* [3]: the sky of sample-environment, outside the scene otherwise */
  memset(materials, 0, sizeof(materials));
  materials[0].num_lobes = 1; /* diffuse_bsdf_node, Cs = 0.73 */
  materials[0].lobes[0].type = PHX_LOBE_DIFFUSE;
  materials[0].lobes[0].weight[0] = materials[0].lobes[0].weight[1] = materials[0].lobes[0].weight[2] = 0.73f;
  materials[1].is_emitter = 1; /* diffuse_emitter_node */
  materials[1].emission[0] = 17.0f; materials[1].emission[1] = 12.0f; materials[1].emission[2] = 4.0f;
  materials[2].num_lobes = 1;
  materials[2].lobes[0].type = PHX_LOBE_DIFFUSE;
  materials[2].lobes[0].weight[0] = 0.63f; materials[2].lobes[0].weight[1] = 0.065f; materials[2].lobes[0].weight[2] = 0.05f;

  phx_face_set sets[3] = {{0, 4, grey_faces}, {1, 2, light_faces}, {2, 2, red_faces}};
  phx_mesh mesh;
  memset(&mesh, 0, sizeof(mesh));
  mesh.vertices = vertices; mesh.num_vertices = 18;
  mesh.faces = faces; mesh.num_faces = 8;
  mesh.flags = PHX_MESH_UV_PER_VERTEX | PHX_MESH_NORMALS_PER_VERTEX;
  mesh.num_sets = 3; mesh.sets = sets;

  phx_scene scene;
  memset(&scene, 0, sizeof(scene));
  scene.num_meshes = 1; scene.meshes = &mesh;
  scene.num_materials = 3; scene.materials = materials;
  scene.environment_material = -1;
  for (int i = 0; i < 4; ++i) scene.camera.to_world[5 * i] = 1.0f; /* camera at the origin looking down -z */
  scene.camera.fov = 1.2f; scene.camera.focal_distance = 1.0f;
  scene.camera.film_width = W; scene.camera.film_height = H;

  phx_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.samples_per_pixel = 8; opt.paths_per_sample = 1; opt.path_depth = 5; opt.device_ordinal = -1;
  int error_estimate = 0, adaptive = 0, denoise = 0, progressive = 0, display = 0, orbit_cameras = 0, orbit_clamp = 0, despeckle = 0, tile_stop = 0, animate_frames = 0;
  float tile_tau = 0.0f;
  phx_adaptive ad;
  memset(&ad, 0, sizeof(ad));
  for (int i = 2; i < argc; ++i)
    if (strcmp(argv[i], "adaptive") == 0 && i + 1 < argc) {  /* the keyword and its number */
      adaptive = 1;
      ad.threshold = (float)atof(argv[i + 1]); ad.floor = 0.0f; ad.min_samples = 4; ad.step = 2;
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else if (strcmp(argv[i], "progressive") == 0 && i + 1 < argc) {
      progressive = atoi(argv[i + 1]);
      if (progressive < 1 || progressive > 1024) progressive = 1;
      const int take = i + 3 < argc && strcmp(argv[i + 2], "tiles") == 0 ? 4 : 2;  /* the keyword, its number and, optionally, `tiles TAU` */
      if (take == 4) { tile_stop = 1; tile_tau = (float)atof(argv[i + 3]); }
      for (int k = i; k + take < argc; ++k) argv[k] = argv[k + take];
      argc -= take; --i;
    } else if (strcmp(argv[i], "orbit") == 0 && i + 1 < argc) {
      orbit_cameras = atoi(argv[i + 1]);
      if (orbit_cameras < 1 || orbit_cameras > 1024) orbit_cameras = 1;
      const int take = i + 2 < argc && strcmp(argv[i + 2], "clamp") == 0 ? 3 : 2;  /* the keyword, its number and, optionally, `clamp` */
      orbit_clamp = take == 3;
      for (int k = i; k + take < argc; ++k) argv[k] = argv[k + take];
      argc -= take; --i;
    } else if (strcmp(argv[i], "animate") == 0 && i + 1 < argc) {  /* the keyword and its number */
      animate_frames = atoi(argv[i + 1]);
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else if (strcmp(argv[i], "display") == 0) {  /* the keyword and, optionally, `auto` */
      const int take = i + 1 < argc && strcmp(argv[i + 1], "auto") == 0 ? 2 : 1;
      display = take;
      for (int k = i; k + take < argc; ++k) argv[k] = argv[k + take];
      argc -= take; --i;
    } else if (strcmp(argv[i], "denoise") == 0 || strcmp(argv[i], "denoise-guided") == 0) {
      denoise = strcmp(argv[i], "denoise") == 0 ? 1 : 2;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else if (strcmp(argv[i], "despeckle") == 0) {
      despeckle = 1;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else if (strcmp(argv[i], "error-estimate") == 0) {
      error_estimate = 1;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else if (strcmp(argv[i], "area-lights") == 0) {  /* taken out of the list: the other arguments keep their places */
      opt.light_sampling = PHX_LIGHTS_BY_AREA;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else if (strcmp(argv[i], "power-lights") == 0) {
      opt.light_sampling = PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else if (strcmp(argv[i], "sample-environment") == 0) {
      static float sky[8 * 4 * 3];
      static phx_texture sky_image;
      for (int k = 0; k < 8 * 4 * 3; ++k) sky[k] = 0.2f;
      sky[(1 * 8 + 5) * 3] = sky[(1 * 8 + 5) * 3 + 1] = 60.0f; sky[(1 * 8 + 5) * 3 + 2] = 40.0f; /* the sun: row 1, column 5 */
      sky_image.width = 8; sky_image.height = 4; sky_image.texels = sky;
      sky_image.filter = PHX_TEX_CLOSEST; sky_image.swrap = PHX_WRAP_PERIODIC; sky_image.twrap = PHX_WRAP_CLAMP;
      materials[3].emission[0] = materials[3].emission[1] = materials[3].emission[2] = 1.0f;
      materials[3].emission_texture = 1; materials[3].emission_mapping = PHX_ENV_LATLONG_Y_UP;
      scene.num_materials = 4; scene.environment_material = 3;
      scene.num_textures = 1; scene.textures = &sky_image;
      opt.light_sampling = PHX_LIGHTS_BY_AREA | PHX_LIGHT_SELECT_BY_POWER | PHX_LIGHT_INCLUDE_ENVIRONMENT;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    }
  if (argc > 2 && strcmp(argv[2], "device-bvh") == 0) opt.bvh_builder = PHX_BVH_DEVICE_LBVH;
  if (argc > 2 && strcmp(argv[2], "host-bvh") == 0) opt.bvh_builder = PHX_BVH_HOST_SAH;

  int n = 0;
  if (phx_discover(&opt, &n) != PHX_OK || n < 1) return fail("phx_discover");
  int num_devices = argc > 3 ? atoi(argv[3]) : 1;
  if (num_devices < 1 || num_devices > 64) num_devices = 1;
  phx_device* devs[64];
  for (int i = 0; i < num_devices; ++i) { /* xpu_t::discover: one device object per GPU (src/xpu.cpp:7-9) */
    opt.device_ordinal = num_devices > 1 ? i % n : -1;
    devs[i] = phx_dev_make(&opt);
    if (!devs[i]) return fail("phx_dev_make");
    if (phx_dev_preprocess(devs[i], &scene) != PHX_OK) return fail("phx_dev_preprocess"); /* every device holds its own copy + BVH */
    if (adaptive && phx_dev_set_adaptive(devs[i], &ad) != PHX_OK) return fail("phx_dev_set_adaptive"); /* the setting is the device's, not the frame's */
    if (tile_stop && !adaptive) { /* frames over a tile subset: their films carry "samples", 0 in a pixel no tile covered.  One round that ends at spp: no decision is ever taken */
      phx_adaptive mark;
      memset(&mark, 0, sizeof(mark));
      mark.threshold = 0.0f; mark.floor = 0.0f; mark.min_samples = opt.samples_per_pixel > 2 ? opt.samples_per_pixel : 2; mark.step = 1;
      if (phx_dev_set_adaptive(devs[i], &mark) != PHX_OK) return fail("phx_dev_set_adaptive");
    }
  }
  if (tile_stop && despeckle) { fprintf(stderr, "despeckle cannot be combined with progressive K tiles TAU: the clamp would read unrendered tiles as taps\n"); return 1; }
  const int samples_channel = adaptive || tile_stop; /* the frame film carries the channel "samples" at float 7 */

  if (animate_frames > 0) { /* moving geometry on the first device, in place of the one frame below */
    const int rc = argc > 1 ? animate(devs[0], &scene, &mesh, animate_frames, argv[1]) : 1;
    for (int i = 0; i < num_devices; ++i) phx_dev_destroy(devs[i]);
    return rc;
  }
  if (orbit_cameras) { /* a path of cameras on the first device, in place of the one frame below */
    const int rc = argc > 1 ? orbit(devs[0], &scene, &opt, orbit_cameras, orbit_clamp, argv[1]) : 1;
    for (int i = 0; i < num_devices; ++i) phx_dev_destroy(devs[i]);
    return rc;
  }
  if (adaptive || denoise || progressive || despeckle) error_estimate = 1; /* the stopping rule, the denoiser and the pooling read the estimate: such a frame must carry it */
  int has_samples = samples_channel; /* the film at hand carries the channel "samples" at float 7 */
  size_t xstride = 4 + (error_estimate ? 3 : 0) + (samples_channel ? 1 : 0); /* primary rgba [, m2 rgb [, samples]] */
  float* film = (float*)calloc((size_t)W * H * xstride, sizeof(float));
  phx_tiles* tiles = phx_tiles_make(W, H, 32, 0, 1); /* ONE job::tiles_t for all devices */
  phx_frame frame;
  memset(&frame, 0, sizeof(frame));
  frame.tiles_user = tiles; frame.next_tile = phx_tiles_next;
  frame.sampler_seed = 7; frame.primary_components = 4;
  frame.host_film = film;                             /* ONE film: tiles are disjoint, so no lock and no reduce */
  frame.moments_channel = (uint32_t)error_estimate;
  for (int i = 0; i < num_devices; ++i)
    if (phx_dev_start(devs[i], &frame) != PHX_OK) return fail("phx_dev_start");
  for (int i = 0; i < num_devices; ++i)
    if (phx_dev_join(devs[i]) != PHX_OK) return fail("phx_dev_join");

  if (despeckle && despeckle_film(devs[0], film, xstride, adaptive, 1)) return 1; /* before anything else reads the film */

  phx_stats st, sum;
  memset(&sum, 0, sizeof(sum));
  for (int i = 0; i < num_devices; ++i) {
    phx_dev_get_stats(devs[i], &st);
    sum.tiles += st.tiles; sum.camera_samples += st.camera_samples; sum.rays_closest += st.rays_closest; sum.rays_shadow += st.rays_shadow;
    sum.bvh_nodes = st.bvh_nodes;
    if (num_devices > 1) printf("device %d (GPU %d): tiles %llu\n", i, i % n, (unsigned long long)st.tiles);
  }
  st = sum;
  printf("tiles %llu camera_samples %llu rays %llu+%llu bvh_nodes %llu\n", (unsigned long long)st.tiles, (unsigned long long)st.camera_samples,
         (unsigned long long)st.rays_closest, (unsigned long long)st.rays_shadow, (unsigned long long)st.bvh_nodes);
  if (error_estimate) {
    /* a pixel's value is a sum of S samples whose centred sum of squares is m2: its variance is estimated by m2 * S / (S - 1) */
    double sum_rse = 0.0; size_t lit = 0;
    for (size_t p = 0; p < (size_t)W * H; ++p) {
      const double S = adaptive ? (double)film[p * xstride + 7] : (double)opt.samples_per_pixel; /* under adaptive sampling: the pixel's own count */
      for (int c = 0; c < 3; ++c) {
        const double v = film[p * xstride + c], m2 = film[p * xstride + 4 + c];
        if (v > 0.0 && S > 1.0) { sum_rse += sqrt(m2 * S / (S - 1.0)) / v; ++lit; }
      }
    }
    printf("error estimate: mean relative standard error %.4f over %llu lit values\n", lit ? sum_rse / (double)lit : 0.0, (unsigned long long)lit);
  }
  if (adaptive) {
    double taken = 0.0;
    for (size_t p = 0; p < (size_t)W * H; ++p) taken += film[p * xstride + 7];
    printf("adaptive: mean samples per pixel %.4f of %u (camera_samples %llu)\n", taken / (double)((size_t)W * H), opt.samples_per_pixel,
           (unsigned long long)st.camera_samples);
  }
  if (progressive) { /* after the join; with several ranks: after the film reduce.  Any device serves: the call reads two films, no scene */
    const size_t xa = 8; /* primary rgba, m2 rgb, samples: an adaptive film's layout */
    float* acc = (float*)calloc((size_t)W * H * xa, sizeof(float));
    if (!acc) return 1;
    phx_accumulate pa;
    memset(&pa, 0, sizeof(pa));
    pa.width = W; pa.height = H; pa.xstride_a = (uint32_t)xa; pa.m2_offset_a = 4; pa.samples_offset_a = 7;
    pa.xstride_b = (uint32_t)xstride; pa.m2_offset_b = 4; pa.samples_offset_b = samples_channel ? 7 : 0; pa.spp_b = opt.samples_per_pixel;
    pa.tau = 0.05f; pa.floor = 0.01f;
    /* tiles TAU: from the second frame on a frame renders only the tiles the tile map of the accumulator leaves open */
    phx_tile_map tm;
    memset(&tm, 0, sizeof(tm));
    tm.width = W; tm.height = H; tm.xstride = (uint32_t)xa; tm.m2_offset = 4; tm.samples_offset = 7; tm.tile_width = tm.tile_height = 32;
    tm.tau = tile_tau; tm.floor = pa.floor;
    const uint32_t num_records = ((W + 31u) / 32u) * ((H + 31u) / 32u);
    phx_tile_record* records = (phx_tile_record*)calloc(num_records, sizeof(phx_tile_record));
    phx_tile* open_list = (phx_tile*)calloc(num_records, sizeof(phx_tile));
    if (!records || !open_list) return 1;
    if (tile_stop) printf("tiles: frame 1 open %u of %u rendered %llu pixels\n", num_records, num_records, (unsigned long long)W * H);
    for (int k = 0; k < progressive; ++k) {
      if (k > 0) { /* the next frame: the same film and queue, a NEW seed (the same seed would be the same samples again) */
        memset(film, 0, (size_t)W * H * xstride * sizeof(float));
        phx_tiles_reset(tiles);
        phx_tiles* open_queue = NULL;
        if (tile_stop) {
          phx_tile_map_summary ts;
          if (phx_dev_film_tile_map(devs[0], &tm, acc, records, &ts) != PHX_OK) return fail("phx_dev_film_tile_map");
          uint32_t open = 0; unsigned long long rendered = 0;
          for (uint32_t r = 0; r < num_records; ++r)
            if (records[r].converged < records[r].tile.w * records[r].tile.h - records[r].invalid || records[r].starved > 0) {
              open_list[open++] = records[r].tile; rendered += (unsigned long long)records[r].tile.w * records[r].tile.h;
            }
          if ((uint64_t)open != ts.open) { fprintf(stderr, "the tile map's summary counts %llu open tiles, its records %u\n", (unsigned long long)ts.open, open); return 1; }
          printf("tiles: frame %d open %u of %u rendered %llu pixels\n", k + 1, open, num_records, rendered);
          if (open == 0) break; /* every tile has converged */
          open_queue = phx_tiles_make_list(open_list, open);
          if (!open_queue) return fail("phx_tiles_make_list");
          frame.tiles_user = open_queue;
        }
        frame.sampler_seed = 7 + (uint64_t)k;
        for (int i = 0; i < num_devices; ++i)
          if (phx_dev_start(devs[i], &frame) != PHX_OK) return fail("phx_dev_start");
        for (int i = 0; i < num_devices; ++i)
          if (phx_dev_join(devs[i]) != PHX_OK) return fail("phx_dev_join");
        if (despeckle && despeckle_film(devs[0], film, xstride, adaptive, k + 1)) return 1;
        if (open_queue) { phx_tiles_free(open_queue); frame.tiles_user = tiles; }
      }
      phx_accumulate_summary ps;
      if (phx_dev_film_accumulate(devs[0], &pa, acc, film, &ps) != PHX_OK) return fail("phx_dev_film_accumulate");
      printf("progressive: frame %d seed %llu samples %llu converged %llu of %llu invalid %llu\n", k + 1, (unsigned long long)frame.sampler_seed,
             (unsigned long long)ps.samples, (unsigned long long)ps.converged, (unsigned long long)ps.pixels, (unsigned long long)ps.invalid);
    }
    free(records); free(open_list);
    free(film);
    film = acc; xstride = xa; has_samples = 1;
  }
  if (denoise) { /* after the join; with several ranks: after the film reduce.  Any device serves: the call reads the film, not the scene */
    phx_denoise dn;
    memset(&dn, 0, sizeof(dn));
    dn.width = W; dn.height = H; dn.xstride = (uint32_t)xstride; dn.m2_offset = 4; dn.samples_offset = has_samples ? 7 : 0;
    dn.spp = opt.samples_per_pixel; dn.iterations = 5; dn.sigma_l = 4.0f; dn.normal_power_log2 = 7;
    double before = 0.0, after = 0.0;
    for (size_t p = 0; p < (size_t)W * H; ++p) for (int c = 0; c < 3; ++c) before += film[p * xstride + 4 + c];
    if (denoise == 2) { /* the guides need the scene: a device that preprocessed it renders them, with the frame's seed */
      float* guides = (float*)calloc((size_t)W * H * 8, sizeof(float));
      phx_guides gp;
      memset(&gp, 0, sizeof(gp));
      gp.sampler_seed = frame.sampler_seed; gp.samples = 4;
      if (!guides || phx_dev_render_guides(devs[0], &gp, guides) != PHX_OK) return fail("phx_dev_render_guides");
      phx_denoise_guides dg;
      memset(&dg, 0, sizeof(dg));
      dg.guides = guides; dg.xstride = 8; dg.flags = PHX_GUIDE_DEMODULATE; dg.albedo_floor = 0.01f;
      if (phx_dev_denoise_guided(devs[0], &dn, &dg, film, film) != PHX_OK) return fail("phx_dev_denoise_guided");
      double cover = 0.0;
      for (size_t p = 0; p < (size_t)W * H; ++p) cover += guides[p * 8 + 3];
      printf("denoise-guided: %u guide samples, mean coverage %.4f\n", gp.samples, cover / (double)((size_t)W * H));
      free(guides);
    } else if (phx_dev_denoise(devs[0], &dn, film, film) != PHX_OK) return fail("phx_dev_denoise");
    for (size_t p = 0; p < (size_t)W * H; ++p) for (int c = 0; c < 3; ++c) after += film[p * xstride + 4 + c];
    printf("denoise: mean m2 %.6g -> %.6g\n", before / (3.0 * W * H), after / (3.0 * W * H));
  }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "wb");
    int ok = f != NULL;
    for (size_t p = 0; ok && p < (size_t)W * H; ++p) ok = fwrite(film + p * xstride, sizeof(float), 4, f) == 4; /* H x W x 4 whatever the film holds */
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    fclose(f);
  }
  if (display && argc > 1) { /* the last step: what the other steps left in `film`, 4 bytes a pixel.  Any device serves: the call reads the film, not the scene */
    phx_display dp;
    phx_display_summary ds;
    memset(&dp, 0, sizeof(dp));
    dp.width = W; dp.height = H; dp.xstride = (uint32_t)xstride;
    dp.flags = PHX_DISPLAY_DITHER | (display == 2 ? PHX_DISPLAY_AUTO_EXPOSURE : 0); dp.tone = PHX_TONE_ACES; dp.scale = 1.0f;
    dp.key = 0.18f; dp.low_q16 = 32768; dp.high_q16 = 62259; dp.min_scale = 1.0f / 4096.0f; dp.max_scale = 4096.0f;
    uint8_t* image = (uint8_t*)malloc((size_t)W * H * 4);
    char* name = (char*)malloc(strlen(argv[1]) + 5);
    if (!image || !name) return 1;
    if (phx_dev_film_display(devs[0], &dp, film, image, &ds, NULL) != PHX_OK) return fail("phx_dev_film_display");
    printf("display: scale %.9g from_histogram %u pixels %llu invalid %llu unlit %llu counted %llu\n", (double)ds.scale, ds.from_histogram,
           (unsigned long long)ds.pixels, (unsigned long long)ds.invalid, (unsigned long long)ds.unlit, (unsigned long long)ds.counted);
    strcpy(name, argv[1]); strcat(name, ".ppm");
    FILE* f = fopen(name, "wb");
    int ok = f != NULL && fprintf(f, "P6\n%d %d\n255\n", W, H) > 0;
    for (size_t p = 0; ok && p < (size_t)W * H; ++p) ok = fwrite(image + 4 * p, 1, 3, f) == 3; /* alpha is dropped */
    if (!ok) { fprintf(stderr, "cannot write %s\n", name); return 1; }
    fclose(f);
    free(name); free(image);
  }
  phx_tiles_free(tiles);
  for (int i = 0; i < num_devices; ++i) phx_dev_destroy(devs[i]);
  free(film);
  return 0;
}
