// What the files that define extern "C" entries of include/rle.h share: the handles behind the opaque pointers,
// the exception-to-return-code guard and the thread's last-error string.
#pragma once
#include <exception>
#include <memory>
#include <string>

#include "replay.h"

struct rle_replay {
  rle::Replay r;
};
struct rle_engine {
  std::unique_ptr<rle::Engine> e;
};

namespace rle {

// What rle_last_error returns on this thread.  One per thread for the whole library: defined in engine.cpp,
// written by guard() in every file.
extern thread_local std::string g_err;

// The engine behind a handle, its rle_step_async burst retired first (Engine::aql_mode; engine.cpp)
Engine& drained(rle_engine* h);

template <class F>
int guard(F&& f) {
  try {
    f();
    return RLE_OK;
  } catch (const Error& err) {
    g_err = err.msg;
    return err.code;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return RLE_ESTATE;
  }
}

}  // namespace rle
