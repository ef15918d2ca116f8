// Index bookkeeping of the profiling timers' pool of event pairs.  Host only (no HIP include): the
// events themselves live in beluga.hip, which records pair p's start and stop, reads the closed
// pairs in resolve_events and creates the events of a pool that has to grow.
//
// A pair is handed out once between two resets: the indices run upwards until the pool is full.
// A full pool is reset -- by the resolve that has read every closed pair -- only while no timer is
// open; while one is open (a launch timer inside its layer's timer) the pool grows instead, so an
// open timer's pair is never handed to another timer before it is read.
#pragma once

#include <cstddef>

namespace expecto {

class EventPairs {
 public:
  enum class Room { kReady, kResolve, kGrow };

  size_t capacity() const { return cap_; }
  size_t open_timers() const { return open_; }

  // What the next open() needs first: nothing, a resolve (reading the closed pairs, then reset())
  // or one more pair (its events created, then grow(1)).
  Room room() const { return next_ < cap_ ? Room::kReady : open_ == 0 ? Room::kResolve : Room::kGrow; }

  // The pair of a new timer, or -1 (the timer then records nothing) if the pool is still full.
  int open() {
    if (next_ >= cap_) return -1;
    ++open_;
    return (int)next_++;
  }
  void close() { --open_; }

  void grow(size_t pairs) { cap_ += pairs; }

  // Every closed pair has been read: hand the pairs out again from 0.  Refused (false) while a
  // timer is open.
  bool reset() {
    if (open_ != 0) return false;
    next_ = 0;
    return true;
  }

 private:
  size_t cap_ = 0, next_ = 0, open_ = 0;
};

}  // namespace expecto
