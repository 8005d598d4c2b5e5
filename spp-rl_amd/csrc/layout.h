// The flat parameter format of every network, once.
//
// Each network lives in ONE contiguous fp32 buffer in state_dict order: an optional leading block of raw
// scalars, then linear layers, each a weight [rows][cols] followed by its bias [rows].  The gradient and Adam
// moment buffers of a net have the same format.  spprl/nets.py and spprl/onpolicy.py state the same formats
// as data for the Python side; tests/test_cpu_layout.py compares the two, tensor by tensor.
//
// Plain C++17, constexpr throughout, nothing from HIP: host code, device code (the constants fold) and a
// plain g++ program read the same header.  Adding a net = one maker here + one *_layout in Python.
#pragma once
#include <cstdint>

namespace spp {

struct NetLayout {
  static constexpr int kMaxLayers = 4;
  int lead = 0;     // raw scalars before the first layer
  int nlayers = 0;  // (0: the handle has no such net; size() = 0)
  int nrows[kMaxLayers] = {}, ncols[kMaxLayers] = {};

  constexpr int rows(int i) const { return nrows[i]; }
  constexpr int cols(int i) const { return ncols[i]; }
  // element offsets of layer i's weight [rows][cols] and bias [rows]
  constexpr int64_t w(int i) const {
    int64_t o = lead;
    for (int k = 0; k < i; ++k) o += (int64_t)nrows[k] * ncols[k] + nrows[k];
    return o;
  }
  constexpr int64_t b(int i) const { return w(i) + (int64_t)nrows[i] * ncols[i]; }
  constexpr int64_t size() const { return nlayers ? w(nlayers) : 0; }
};

// layer indices that are not simply fc1, fc2, fc3 = 0, 1, 2
constexpr int kFcProb = 2, kFcScale = 3;         // SAC actor heads
constexpr int kBacmFc21 = 2, kBacmFc3 = 3;       // BasicAcM
constexpr int kBacmT = 0, kBacmT1 = 1;           // BasicAcM: offsets of t and t1 [ac] in its leading block

// SAC_Actor (rltoolkit/algorithms/sac/models.py:8-22): fc1, fc2, fc_prob, fc_scale
constexpr NetLayout sac_actor_layout(int ob, int aout) {
  return NetLayout{0, 4, {256, 256, aout, aout}, {ob, 256, 256, 256}};
}
// DDPG Actor (rltoolkit/algorithms/ddpg/models.py:5-22): fc1, fc2, fc3 (-> aout)
constexpr NetLayout ddpg_actor_layout(int ob, int aout) { return NetLayout{0, 3, {256, 256, aout}, {ob, 256, 256}}; }
// SAC_Critic (rltoolkit/algorithms/sac/models.py:72-80), also DDPG's: fc1 on cin = ob + action, fc2, fc3 (-> 1)
constexpr NetLayout critic_layout(int cin) { return NetLayout{0, 3, {256, 256, 1}, {cin, 256, 256}}; }
// AcM (rltoolkit/basic_model.py:108-117): fc1 (-> 64), fc2 (-> 32), fc3 (-> ac)
constexpr NetLayout acm_layout(int in, int ac) { return NetLayout{0, 3, {64, 32, ac}, {in, 64, 32}}; }
// BasicAcM (rltoolkit/acm/models/basic_acm.py:11-21): t, t1 [ac], then fc1 (-> 100), fc2 (-> 50),
// fc21 (in -> 50), fc3 (-> ac); the module's own parameters precede its submodules' in state_dict
constexpr NetLayout bacm_layout(int in, int ac) {
  return NetLayout{1 + ac, 4, {100, 50, 50, ac}, {in, 100, in, 50}};
}
// on-policy Actor (rltoolkit/basic_model.py:14-21): log_scale [aout], then fc1 (-> 64), fc2 (-> 64), fc3 (-> aout)
constexpr NetLayout onp_actor_layout(int ob, int aout) { return NetLayout{aout, 3, {64, 64, aout}, {ob, 64, 64}}; }
// on-policy Critic (rltoolkit/basic_model.py:62-70): fc1 (-> 64), fc2 (-> 64), fc3 (-> 1)
constexpr NetLayout onp_critic_layout(int ob) { return NetLayout{0, 3, {64, 64, 1}, {ob, 64, 64}}; }

}  // namespace spp
