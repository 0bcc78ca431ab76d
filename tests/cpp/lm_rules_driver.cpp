// lm_rules_driver.cpp — csrc/liw_lm_rules.hpp on the host, for tests/test_lm_rules.py: one query per line of standard input, one answer per
// line of standard output.  Doubles travel as C hexadecimal floating-point text in both directions (exact; strtod also reads inf and nan).
//   const                                   -> the constants, in the order of the header
//   cand  step_norm x_norm x_cost cand_cost -> lm_candidate_term
//   step  x_cost cand_cost model radius dec -> rho, lm_accepts, then radius / dec / reuse after lm_step_accepted or lm_step_rejected
//   grad  first last_successful gmax above  -> lm_gradient_term
//   cap   iteration max_iters fresh         -> lm_cap_reached
//   valid solved model_cost_change          -> lm_step_valid
//   gives invalid_steps_before              -> lm_gives_up
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../2dliw-slam_amd/csrc/liw_lm_rules.hpp"

int main() {
    using namespace liw;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char* p = line;
        char op[16] = {0};
        int used = 0;
        if (sscanf(p, "%15s%n", op, &used) != 1) continue;
        p += used;
        double v[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < 5; ++k) { char* e; v[k] = strtod(p, &e); if (e == p) break; p = e; }
        if (!strcmp(op, "const")) {
            printf("%a %a %a %a %a %a %a %a %a %d %a\n", kMinDiag, kMaxDiag, kMinRelDec, kFuncTol, kGradTol, kParamTol, kMaxRadius, kMinRadius,
                   kInitRadius, kMaxInvalidSteps, kFailedEvalCost);
        } else if (!strcmp(op, "cand")) {
            printf("%d\n", lm_candidate_term(v[0], v[1], v[2], v[3]));
        } else if (!strcmp(op, "step")) {
            const double rho = (v[0] - v[1]) / v[2];
            double radius = v[3], dec = v[4];
            int reuse = -1;
            const bool acc = lm_accepts(rho);
            if (acc) lm_step_accepted(rho, radius, dec, reuse);
            else lm_step_rejected(radius, dec, reuse);
            printf("%a %d %a %a %d\n", rho, acc ? 1 : 0, radius, dec, reuse);
        } else if (!strcmp(op, "grad")) {
            printf("%d\n", lm_gradient_term(v[0] != 0.0, v[1] != 0.0, v[2], v[3] != 0.0));
        } else if (!strcmp(op, "cap")) {
            printf("%d\n", lm_cap_reached((int)v[0], (int)v[1], v[2] != 0.0) ? 1 : 0);
        } else if (!strcmp(op, "valid")) {
            printf("%d\n", lm_step_valid(v[0] != 0.0, v[1]) ? 1 : 0);
        } else if (!strcmp(op, "gives")) {
            printf("%d\n", lm_gives_up((int)v[0]) ? 1 : 0);
        } else {
            fprintf(stderr, "lm_rules_driver: unknown query '%s'\n", op);
            return 2;
        }
    }
    return 0;
}
