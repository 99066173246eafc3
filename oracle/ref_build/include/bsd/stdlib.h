/* Stand-in for libbsd's <bsd/stdlib.h>: the units built here use nothing beyond the C library's
 * <stdlib.h>. */
#ifndef ORC_REF_STANDIN_BSD_STDLIB_H
#define ORC_REF_STANDIN_BSD_STDLIB_H
#include <stdlib.h>
#endif
