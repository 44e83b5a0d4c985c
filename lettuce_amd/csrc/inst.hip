// Every kernel object of the library: one unit (-DLT_UNIT=<tag>: dispatch.hpp, LT_UNITS) and one of its parts
// (-DLT_PART=<name>: unit.inc).  The Makefile lists which unit has which parts.
#include "unit.inc"
