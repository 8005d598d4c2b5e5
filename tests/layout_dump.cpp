// Prints the flat-buffer formats of spp-rl_amd/csrc/layout.h for tests/test_cpu_layout.py (plain g++, no HIP).
//   layout_dump MAKER A B [MAKER A B ...]     (B is ignored by the one-argument makers)
// Per net:   net MAKER A B lead LEAD size SIZE
// per layer: tensor INDEX OFFSET ROWS COLS    (weight: index 2 i, bias: index 2 i + 1 with COLS 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../spp-rl_amd/csrc/layout.h"

using spp::NetLayout;

// the header is constexpr throughout: these fold at compile time
static_assert(spp::sac_actor_layout(11, 11).size() == 256 * 11 + 256 + 65536 + 256 + 2 * (11 * 256 + 11), "sac actor");
static_assert(spp::onp_actor_layout(17, 6).w(0) == 6 && spp::onp_actor_layout(17, 6).b(2) == 6 + 64 * 17 + 64 + 4096 + 64 + 6 * 64,
              "on-policy actor");
static_assert(NetLayout{}.size() == 0, "no net");

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: layout_dump MAKER A B [MAKER A B ...]\n");
    return 2;
  }
  for (int k = 1; k + 2 < argc; k += 3) {
    const char* mk = argv[k];
    const int a = std::atoi(argv[k + 1]), b = std::atoi(argv[k + 2]);
    NetLayout L;
    if (!std::strcmp(mk, "sac_actor")) L = spp::sac_actor_layout(a, b);
    else if (!std::strcmp(mk, "ddpg_actor")) L = spp::ddpg_actor_layout(a, b);
    else if (!std::strcmp(mk, "critic")) L = spp::critic_layout(a);
    else if (!std::strcmp(mk, "acm")) L = spp::acm_layout(a, b);
    else if (!std::strcmp(mk, "bacm")) L = spp::bacm_layout(a, b);
    else if (!std::strcmp(mk, "onp_actor")) L = spp::onp_actor_layout(a, b);
    else if (!std::strcmp(mk, "onp_critic")) L = spp::onp_critic_layout(a);
    else {
      std::fprintf(stderr, "layout_dump: no maker '%s'\n", mk);
      return 2;
    }
    std::printf("net %s %d %d lead %d size %lld\n", mk, a, b, L.lead, (long long)L.size());
    if (!std::strcmp(mk, "bacm")) std::printf("bacm_t %d bacm_t1 %d\n", spp::kBacmT, spp::kBacmT1);
    for (int i = 0; i < L.nlayers; ++i) {
      std::printf("tensor %d %lld %d %d\n", 2 * i, (long long)L.w(i), L.rows(i), L.cols(i));
      std::printf("tensor %d %lld %d 0\n", 2 * i + 1, (long long)L.b(i), L.rows(i));
    }
  }
  return 0;
}
