// crmath_driver.cpp — csrc/liw_crmath.hpp on the host, for tests/test_crmath.py and tests/test_gpu_crmath.py: one query per line of standard
// input, "<op> <a> <b>" with op 0 sin(a), 1 cos(a), 2 atan2(a, b) and a, b the bit patterns of the doubles in hexadecimal; one answer per line
// of standard output, the bit pattern of the result.  Compile without contraction, as the library's host code is.
#include <cstdio>
#include <cstring>

#include "../../2dliw-slam_amd/csrc/liw_crmath.hpp"

int main() {
    int op;
    unsigned long long ua, ub;
    while (scanf("%d %llx %llx", &op, &ua, &ub) == 3) {
        double a, b, r;
        memcpy(&a, &ua, 8);
        memcpy(&b, &ub, 8);
        if (op == 0) r = liw_cr::cr_sin(a);
        else if (op == 1) r = liw_cr::cr_cos(a);
        else if (op == 2) r = liw_cr::cr_atan2(a, b);
        else { fprintf(stderr, "crmath_driver: unknown op %d\n", op); return 2; }
        unsigned long long ur;
        memcpy(&ur, &r, 8);
        printf("%016llx\n", ur);
    }
    return 0;
}
