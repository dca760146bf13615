// The one registry of live allocations (memory.h live_allocs): DevMem, PinMem and Engine::prog_options share it.
#include "memory.h"

namespace rle {

AllocRegistry& live_allocs() {
  static AllocRegistry r;
  return r;
}

}  // namespace rle
