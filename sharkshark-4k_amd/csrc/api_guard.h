// guard(): the body of every extern "C" entry point (api.cpp, api_dev.cpp).  What f throws becomes the return code and the text of
// ss4k_last_error(); success clears that text.
#pragma once
#include "common.h"

namespace ss4k {
void clear_error();   // api.cpp, next to set_error
template <typename F> static int guard(F&& f) {
  try { f(); clear_error(); return SS4K_OK; }
  catch (const Error& e) { set_error("%s", e.what()); return e.code; }
  catch (const std::bad_alloc&) { set_error("out of host memory"); return SS4K_ENOMEM; }
  catch (const std::exception& e) { set_error("%s", e.what()); return SS4K_EINVAL; }
}
}  // namespace ss4k
