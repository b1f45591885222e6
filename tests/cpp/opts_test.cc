// The option table (syzkaller_amd/csrc/sg_opts.h) printed from a plain C++
// build, one row a line: index, name, default, lo, hi.
#include <cstdio>

#include "sg_opts.h"

int main() {
  for (int i = 0; i < kOptCount; i++)
    printf("%d %s %lld %lld %lld\n", i, kSgOpts[i].name, (long long)kSgOpts[i].def, (long long)kSgOpts[i].lo,
           (long long)kSgOpts[i].hi);
  return 0;
}
