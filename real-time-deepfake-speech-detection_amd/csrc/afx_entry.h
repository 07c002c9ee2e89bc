// What the C entry points of include/afx.h share, in whichever unit they are defined (internal to libafx): the error
// store behind afx_last_error and the way a launcher's refusal becomes the entry point's return value.
#pragma once
#include <cstdio>

namespace afx {

// records the message afx_last_error returns on the calling thread; returns 1 (afx_engine.hip)
int fail(const char* fmt, ...);

// the value of an entry point from a launcher's result: nullptr = launched (0), else the refusal or HIP's error string
#define KRET(expr)                       \
  do {                                   \
    const char* m_ = (expr);             \
    return m_ ? fail("%s", m_) : 0;      \
  } while (0)

// a refusal in the name of the entry point `who` (the launch cores that serve several entry points)
inline const char* launch_msg(const char* who, const char* what) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return msg;
}

}  // namespace afx
