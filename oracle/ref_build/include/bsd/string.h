/* Stand-in for libbsd's <bsd/string.h>: the C library's <string.h> plus the two prototypes of
 * strlcpy(3) / strlcat(3), as their man page gives them.  ref_harness.c defines both where the
 * C library has none. */
#ifndef ORC_REF_STANDIN_BSD_STRING_H
#define ORC_REF_STANDIN_BSD_STRING_H
#include <string.h>
size_t strlcpy(char *dst, const char *src, size_t size);
size_t strlcat(char *dst, const char *src, size_t size);
#endif
