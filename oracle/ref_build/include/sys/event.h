/* Stand-in for the BSD <sys/event.h> (kqueue), which Linux does not have.  The units built here
 * never name struct kevent, so nothing is declared. */
#ifndef ORC_REF_STANDIN_SYS_EVENT_H
#define ORC_REF_STANDIN_SYS_EVENT_H
#endif
