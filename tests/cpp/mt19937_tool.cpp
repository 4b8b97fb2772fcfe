// prints the first N outputs of std::mt19937(seed), one per line (tests/test_segment_host.py compares the NumPy
// restatement of boost::mt19937 with it)
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char** argv) {
  const unsigned long seed = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 5489ul;
  const int n = argc > 2 ? std::atoi(argv[2]) : 10;
  std::mt19937 e(static_cast<std::mt19937::result_type>(seed));
  for (int i = 0; i < n; i++) std::printf("%u\n", static_cast<unsigned>(e()));
  return 0;
}
