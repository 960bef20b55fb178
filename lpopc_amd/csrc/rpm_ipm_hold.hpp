// rpm_ipm_hold.hpp — what a device solver (rpm_ipm, rpm_ipm_solver.hpp) holds between two calls, and so what may be called after
// what: the rule every entry point that injects or consumes a state goes by (the table in DESIGN.md f-2).  No HIP, no engine:
// tests/native/ipm_hold_test.cpp walks every call sequence of it with the host compiler.
#pragma once

namespace rpm {

struct IpmHold {
  enum State {
    Nothing,     // no usable state: fresh, a solve that failed, the factor hooks, after the step update
    Started,     // rpm_ipm_debug_start was the last call: D.v, D.lam, D.zL, D.zU, D.vl, D.vu hold a start state
    Held,        // a finished solve, or an rpm_ipm_debug_pass that left no direction: the same arrays hold its state
    Direction,   // rpm_ipm_debug_pass(stage 3) left instances running: D.K holds the factors, D.rhs and D.dv ... their direction
    Searched     // rpm_ipm_debug_line_search has run: trial points stand, the state is no longer a start's or a pass's
  };
  State state = Nothing;
  bool solved = false;   // D.zL / D.zU hold a solve's multipliers (independent of `state`: the factor hooks leave them alone)

  // ---- what the refusals ask
  bool pass_allowed() const { return state == Started; }
  bool line_search_allowed() const { return state == Direction || state == Searched; }
  bool update_allowed() const { return state == Searched; }
  bool holds_state() const { return state == Started || state == Held || state == Direction; }   // sensitivities may be taken at it
  bool multipliers_ready() const { return solved; }

  // ---- the events, named after the call that causes them; one that needs a state is the caller's to refuse first
  void solve_begins() { state = Nothing; }
  void solve_ends() { state = Held; solved = true; }
  void overwritten() { state = Nothing; }                    // the factor hooks and the limited-memory step hook: their own data in D
  void start_begins() { state = Nothing; solved = false; }   // (a start that fails on the device leaves this)
  void start_ends() { state = Started; }
  void pass_begins() { state = Held; }
  void pass_ends(bool direction_stands) { state = direction_stands ? Direction : Held; }
  bool line_search_begins() {                                // -> the first round ever on this direction
    const bool first = state == Direction;
    state = Nothing;
    return first;
  }
  void line_search_ends() { state = Searched; }
  void updated() { state = Nothing; }
  void sensitivities_taken() { if (state == Direction) state = Held; }   // D.K and D.rhs are rewritten: the state stays, a direction does not
};

}  // namespace rpm
